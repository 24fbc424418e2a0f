"""CPU side of the pre-processing edges (tests/preprocess_edges.py): the constants of the table are read out of the
sources as text (a moved threshold fails here until the table follows), the two reference functions are held against
oracle/preprocess.py wherever the oracle can serve, every construction is checked for what it is there for, and the
voxel wrapper's grid arithmetic (`preprocess._voxel_grid`) is tested without a device."""
import os
import re

import numpy as np
import pytest

from oracle import preprocess as OP
from tests import preprocess_edges as PE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "s4g_release_amd", "csrc")


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _one(pattern, text, what):
    found = re.findall(pattern, text, flags=re.M)
    assert len(found) == 1, "%s: expected exactly one match of %r, found %d" % (what, pattern, len(found))
    return found[0]


def _body(text, signature):
    start = text.index(signature)
    return text[start:text.index("\n}", start)]


# --------------------------------------------------------------------------------------------------------- constants
def test_the_constants_are_the_sources():
    grid, pp, bq, rs = _read("grid.h"), _read("preprocess.hip"), _read("ball_query.hip"), _read("radix_sort.hip")
    for name in ("GR_DIM", "GR_COORD_LIMIT", "GR_MAX_POINTS", "GR_BUILD_THREADS"):
        assert int(_one(r"^constexpr int %s = (\d+);" % name, grid, name)) == getattr(PE, name), name
    _one(r"fabsf\(__fmul_rn\(__fsub_rn\(v, o\), inv_h\)\) < \(float\)\(GR_COORD_LIMIT - 1\);", grid, "grid_coord_ok")
    _one(r"return \(int\)floorf\(__fmul_rn\(__fsub_rn\(v, o\), inv_h\)\);", grid, "grid_coord")
    entry = _body(pp, 'extern "C" int s4g_radius_outlier_mask_f32(')
    num, den = _one(r"const float h = radius \* \(1\.0f \+ (\d+\.\d+)f / (\d+\.\d+)f\);", entry, "cell edge")
    assert float(num) / float(den) == PE.GR_WIDEN
    _one(r"const float inv_h = 1\.0f / h;", entry, "inv_h")
    _one(r"const float r2 = radius \* radius;", entry, "r2")
    assert float(_one(r"if \(N > GR_MAX_POINTS \|\| !\(radius < ([0-9e.]+)f\)\)", entry, "scan switch")) == PE.RADIUS_SCAN_FROM
    assert int(_one(r"const int threads = (\d+),", entry, "radius launch block")) == PE.VOXEL_THREADS
    _one(r"if \(N <= 0 \|\| N > s4g::GR_MAX_POINTS\) return 0;", pp, "radius workspace size")
    assert int(_one(r"^constexpr int PP_THREADS = (\d+);", pp, "PP_THREADS")) == PE.PP_THREADS
    voxel = _body(pp, 'extern "C" int s4g_voxel_down_sample_f32(')
    assert int(_one(r"const int threads = (\d+),", voxel, "voxel launch block")) == PE.VOXEL_THREADS
    _one(r"while \(bits < 32 && \(1ull << bits\) < cells\) \+\+bits;", voxel, "key width")
    count = _body(pp, "__global__ void radius_count_kernel(")
    _one(r"if \(x0 <= GR_DIM - 3\) \{", count, "x-run wrap")
    assert len(re.findall(r"dist2<FMAD>\([^)]*\) < r2 \? 1 : 0;", count)) == 3
    _one(r"keep\[j\] = cnt > nb \? 1 : 0;", count, "threshold")
    build = _body(bq, "int launch_grid_build(")
    ladder = re.findall(r"if \(N <= (\d+) \* GR_BUILD_THREADS\) S4G_GB_LAUNCH\((\d+)\);", build)
    assert [(int(a), int(b)) for a, b in ladder] == [(p, p) for p in PE.GR_BUILD_LADDER]
    tile = _one(r"^constexpr int RS_CHUNKS = (\d+);", rs, "RS_CHUNKS")
    assert 64 * int(tile) * (int(_one(r"^constexpr int RS_THREADS = (\d+),", rs, "RS_THREADS")) // 64) == PE.SORT_TILE


def test_the_ladders_stand_on_the_thresholds():
    n = set(PE.RADIUS_LADDER_N)
    for t in (PE.VOXEL_THREADS, PE.GR_MAX_POINTS) + tuple(p * PE.GR_BUILD_THREADS for p in PE.GR_BUILD_LADDER):
        assert {t, t + 1} <= n, t
    assert {1, 2, PE.VOXEL_THREADS - 1, PE.GR_MAX_POINTS - 1} <= n
    v = set(PE.VOXEL_N)
    for t in (PE.VOXEL_THREADS, PE.SORT_TILE):
        assert {t - 1, t, t + 1} <= v, t
    assert 2 * PE.SORT_TILE + 1 in v
    c = set(PE.CROP_N)
    for t in (PE.WAVE, PE.PP_THREADS, 2 * PE.PP_THREADS):
        assert {t - 1, t, t + 1} <= c, t
    assert {0, 1, 3 * PE.PP_THREADS + 1} <= c
    ids = [i for i, _, _ in PE.radius_cases()]
    assert len(set(ids)) == len(ids)
    assert set(PE.FMAD_CASES) <= set(ids) and PE.TWICE_CASE in ids


# --------------------------------------------------------------------------------------------------------- references
def test_counts_ref_equals_the_oracle_on_every_small_scene():
    seen = set()
    for name, get, _ in PE.radius_cases():
        s = get()
        if s.n > 8193 or id(s) in seen:
            continue
        seen.add(id(s))
        with np.errstate(all="ignore"):           # the oracle subtracts inf from inf and squares 1e20 in fp32
            want = OP.radius_neighbour_counts(s.points, s.radius)
        assert np.array_equal(s.counts(), want), name
    assert len(seen) >= 25


@pytest.mark.parametrize("n", [300, 4000, 12000])
def test_counts_ref_equals_the_oracle_on_table_top_clouds(n):
    p = PE.tabletop(n, scene=3)
    for r in (0.01, 0.02, 0.05) if n < 12000 else (0.02,):
        assert np.array_equal(PE.counts_ref(p, r), OP.radius_neighbour_counts(p, r)), r


def test_fmad_reference_rounds_once():
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(3)
    d = (rng.standard_normal((3, 3000)) * 0.0115).astype(np.float32)
    d[:, 0] = np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -30), 0.0   # dx dx is a tie a later tiny term breaks
    for k in range(d.shape[1]):
        dx, dy, dz = (float(v) for v in d[:, k])
        want = libm.fmaf(dz, dz, libm.fmaf(dy, dy, float(np.float32(dx) * np.float32(dx))))
        assert PE.fmad_dist2_exact(*d[:, k]).tobytes() == np.float32(want).tobytes(), k
    # counts under fmad: the same as counting over the exact fused distance of every candidate pair
    s = PE.pair_scene()
    inside = PE.pair_dist2(s, fmad=True) < np.float32(s.radius) * np.float32(s.radius)
    assert np.array_equal(s.counts(True), 1 + np.repeat(inside, 2))


def test_voxel_ref_equals_the_oracle_on_the_wrappers_grid():
    scenes = [PE.voxel_fill_scene(n, fill) for n in PE.VOXEL_N for fill in PE.VOXEL_FILLS]
    scenes += [PE.voxel_bits_scene(k)[:2] for k in range(len(PE.BITS_LADDER))] + [PE.voxel_bounds_scene()]
    for pts, v in scenes:
        origin, dims = OP.voxel_grid(pts, v)
        ref = OP.voxel_down_sample(pts, v)
        got = PE.voxel_ref(pts, v, origin, dims)
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes()


# --------------------------------------------------------------------------------------------------------- radius scenes
def test_every_ladder_entry_separates_points():
    for n in PE.RADIUS_LADDER_N:
        s = PE.ladder_scene(n)
        assert s.n == n and np.isfinite(s.points).all()
        if n <= 2:          # both points alike (see the table): the row runs at both outcomes
            assert PE.ladder_nbs(n) == [0, n] and (s.counts() > 0).all() and not (s.counts() > n).any()
            continue
        share = float((s.counts() > PE.LADDER_NB).mean())
        print("ladder N=%d r=%.6f nb=%d keeps %.1f %%" % (n, s.radius, PE.LADDER_NB, 100 * share))
        assert 0.10 <= share <= 0.90, (n, share)
        assert s.radius < PE.RADIUS_SCAN_FROM
        assert np.abs(PE.cells_of(s.points, s.radius)).max() < PE.GR_COORD_LIMIT - 1      # the grid branch, no flag


def test_torus_scene_is_what_it_says():
    s = PE.torus_scene()
    assert 2500 <= s.n <= 3500
    cells = PE.cells_of(s.points, s.radius)
    assert np.array_equal(cells, s.cell)                                   # every point fell into its intended cell
    assert cells[:, 0].tolist() == [0, 0, 0]
    for axis in range(3):                                                  # the lattice reaches 40 cells both ways
        assert cells[axis].min() <= -PE.TORUS_REACH and cells[axis].max() >= PE.TORUS_REACH
    assert np.abs(cells).max() < PE.GR_COORD_LIMIT - 1
    base = s.alias_of < 0
    core = (s.kind == "core") & base
    assert sorted(set(int(v) % PE.GR_DIM for v in cells[0, core])) == [0, 1, 30, 31]
    assert set(int(v) for v in cells[0, core]) == set(PE.TORUS_X_CELLS)
    for sign, k in ((-1, "probe-"), (1, "probe+")):                        # the probes sit in the x-neighbour cells
        assert ((s.kind == k) & base).sum() == len(PE.TORUS_X_CELLS) * len(PE.TORUS_CORE_SIZES)
    # aliases: exactly 32 cells away along one axis, equal coordinates mod 32, three per clustered point
    al = np.nonzero(~base)[0]
    delta = cells[:, al] - cells[:, s.alias_of[al]]
    assert (np.abs(delta).sum(axis=0) == PE.GR_DIM).all()
    assert (delta[s.shift_axis[al], np.arange(len(al))] == PE.GR_DIM).all()
    assert (np.mod(delta, PE.GR_DIM) == 0).all()
    clustered = np.isin(s.kind, ("core", "probe-", "probe+")) & base
    assert np.array_equal(np.bincount(s.alias_of[al], minlength=s.n)[clustered], np.full(clustered.sum(), 3))
    assert set(s.shift_axis[al].tolist()) == {0, 1, 2}
    # the counts: core points see core + 2, probes core + 1, aliases the same as their base
    c = s.counts()
    assert set(c[s.kind == "core"].tolist()) == {PE.TORUS_NB, PE.TORUS_NB + 1, PE.TORUS_NB + 2, PE.TORUS_NB + 3}
    for k in ("probe-", "probe+"):
        assert set(c[s.kind == k].tolist()) == {PE.TORUS_NB - 1, PE.TORUS_NB, PE.TORUS_NB + 1, PE.TORUS_NB + 2}
    for x in (29, 30, 31, 0, 1, 2):               # a kept and a dropped probe in every x cell around the wrap
        sel = np.isin(s.kind, ("probe-", "probe+")) & (np.mod(cells[0], PE.GR_DIM) == x)
        assert (c[sel] == PE.TORUS_NB).any() and (c[sel] == PE.TORUS_NB + 1).any(), x
    assert np.array_equal(c[al], c[s.alias_of[al]])
    # what a kernel that counted the whole slot (no distance test across 32 cells) would see differs
    slot = np.mod(cells, PE.GR_DIM)
    assert len(np.unique(slot.T, axis=0)) < len(np.unique(cells.T, axis=0))


def test_cell27_scene_fills_27_cells():
    for which, centre in PE.CELL27_CENTRES.items():
        s = PE.cell27_scene(which)
        cells = PE.cells_of(s.points, s.radius)[:, 1:]
        assert cells[:, 0].tolist() == list(centre)
        assert len(np.unique(cells.T, axis=0)) == 27
        assert np.abs(cells - cells[:, :1]).max() == 1
        c = s.counts()
        assert c[1] == 27 and (c[2:] < 27).all() and c[0] == 1
    assert min(PE.CELL27_CENTRES["negative"]) < 0 and max(PE.CELL27_CENTRES["negative"]) < 0


def test_pair_scene_straddles_r2():
    s = PE.pair_scene()
    r2 = np.float32(s.radius) * np.float32(s.radius)
    d, df = PE.pair_dist2(s), PE.pair_dist2(s, fmad=True)
    exact, disagree = int((d == r2).sum()), int(((d < r2) != (df < r2)).sum())
    print("pair scene: %d inside, %d at r^2, %d outside; strict and fmad disagree on %d"
          % ((d < r2).sum(), exact, (d > r2).sum(), disagree))
    assert exact >= 8 and disagree >= 4
    assert (d < r2).mean() >= 0.25 and (d > r2).mean() >= 0.25
    assert np.array_equal(s.counts(), 1 + np.repeat(d < r2, 2))             # the pairs are isolated
    assert np.array_equal(s.counts(True), 1 + np.repeat(df < r2, 2))


def test_pair_variants_reach_the_other_two_loops():
    base = PE.pair_scene()
    flier, scan = PE.pair_variant_scene("flier"), PE.pair_variant_scene("scan")
    assert flier.n == base.n + 1 and PE.cells_of(flier.points, flier.radius)[0, -1] > PE.GR_COORD_LIMIT - 1
    assert scan.n == PE.GR_MAX_POINTS + 1
    for fmad in (False, True):                    # the added points are far from every pair
        assert np.array_equal(flier.counts(fmad)[:base.n], base.counts(fmad)) and flier.counts(fmad)[-1] == 1
    assert np.array_equal(scan.counts()[:base.n], base.counts())


def test_fallback_scenes_leave_the_exactness_range():
    lim = PE.GR_COORD_LIMIT - 1
    with np.errstate(invalid="ignore"):
        for which in PE.FALLBACK_KINDS:
            s = PE.fallback_scene(which)
            cells = PE.cells_of(s.points, s.radius)
            assert not (np.abs(cells) < lim).all(), which                   # NaN compares false: flagged as well
        flier = PE.cells_of(PE.fallback_scene("flier").points, PE.TORUS_RADIUS)
    assert np.isfinite(flier).all() and flier[0, -1] == PE.FLIER_CELLS > lim
    assert np.abs(flier[:, :-1]).max() < lim
    assert np.isnan(PE.fallback_scene("nan-origin").points[0, 0])
    assert not PE.fallback_scene("nan-origin").counts()[0]
    assert np.isfinite(PE.fallback_scene("nan-only").points).sum() == 3 * PE.torus_scene().n - 1


def test_degenerate_radii_are_what_they_say():
    cases = {name: (s, nbs) for name, s, nbs in PE.degenerate_cases()}
    f = np.float32
    with np.errstate(over="ignore", under="ignore"):
        assert np.isfinite(f(1e19) * f(1e19)) and np.isinf(f(1e20) * f(1e20))
        r2 = f(1e-20) * f(1e-20)
        assert 0 < r2 < np.finfo(np.float32).tiny                           # a denormal
        assert f(1e-23) * f(1e-23) == 0
    n = cases["r1e19"][0].n
    assert (cases["r1e19"][0].counts() == n).all() and (cases["r1e20"][0].counts() == n).all()
    c = cases["r1e19-nan"][0].counts()
    assert c[17] == 0 and (np.delete(c, 17) == n - 1).all()
    assert sorted(set(cases["r1e19"][1])) == [0, n - 1, n, 2 ** 31 - 1] == sorted(set(cases["grid-nb"][1]))
    s = cases["r1e-20"][0]
    assert np.array_equal(s.counts(), s.group) and set(s.group.tolist()) == {1, 2, 3}
    assert (cases["r1e-20-one-cell"][0].counts() == 5).all()
    assert not cases["r1e-23"][0].counts().any() and not cases["r1e-23-one-cell"][0].counts().any()


# --------------------------------------------------------------------------------------------------------- voxel scenes
def test_voxel_fills_are_what_they_say():
    for n in PE.VOXEL_N:
        for fill in PE.VOXEL_FILLS:
            pts, v = PE.voxel_fill_scene(n, fill)
            assert pts.shape == (3, n) and np.isfinite(pts).all()
            origin, dims = OP.voxel_grid(pts, v)
            idx = np.floor(((pts - origin[:, None]).astype(np.float32) / np.float32(v)).astype(np.float32)).astype(int)
            assert (idx >= 0).all() and (idx < dims[:, None]).all()          # no clamp through the wrapper
            cells = len(np.unique(idx.T, axis=0))
            if fill == "own-cell":
                assert cells == n
                assert np.array_equal(pts.astype(np.float64), origin[:, None] + (idx + 0.5) * v)   # cell centres, exact
                assert n < 3 or not np.array_equal(np.lexsort(idx), np.arange(n))                   # shuffled
            elif fill == "one-cell":
                assert cells == 1
            else:
                sizes = np.unique(idx.T, axis=0, return_counts=True)[1]
                assert n < 303 or {1, 2, 300} <= set(sizes.tolist())
                # the mean of a 300-point cell in fp32 is not the double mean: the case can tell them apart
                if n >= 300:
                    ref = OP.voxel_down_sample(pts, v)
                    key = (idx[2] * int(dims[1]) + idx[1]) * int(dims[0]) + idx[0]
                    f32 = np.stack([[pts[a, key == k].sum(dtype=np.float32) / np.float32((key == k).sum())
                                     for k in np.unique(key)] for a in range(3)]).astype(np.float32)
                    assert f32.shape == ref.shape and not np.array_equal(f32, ref)


def test_bits_ladder_gives_the_intended_key_widths():
    assert [b for _, _, b in PE.BITS_LADDER] == [1, 1, 8, 8, 9, 16, 17, 24, 25, 32]
    for k, (dims, v, bits) in enumerate(PE.BITS_LADDER):
        pts, v2, d2 = PE.voxel_bits_scene(k)
        origin, got = OP.voxel_grid(pts, v)
        assert v2 == v and d2 == dims and tuple(int(x) for x in got) == dims      # the wrapper's grid IS the intended one
        assert int(np.prod(np.array(dims, dtype=np.int64))) == PE.BITS_CELLS[k] and PE.key_bits(dims) == bits
        idx = np.floor(((pts - origin[:, None]).astype(np.float32) / np.float32(v)).astype(np.float32)).astype(np.int64)
        key = (idx[2] * dims[1] + idx[1]) * dims[0] + idx[0]
        assert key.min() == 0 and key.max() == PE.BITS_CELLS[k] - 1                 # the extreme corners
        assert len(np.unique(key)) < len(key)                                       # some cells hold two points
    assert key.max() >= 2 ** 31 and (key >= 2 ** 31).sum() >= 4                     # the last entry: signed keys would sort first


def test_bounds_and_clamp_scenes():
    pts, v = PE.voxel_bounds_scene()
    origin, dims = OP.voxel_grid(pts, v)
    assert origin.tolist() == [1.0, -1.0, 0.0]
    on = below = above = 0
    for a in range(3):
        bounds = (origin[a] + np.float32(v) * np.arange(1, 5, dtype=np.float32)).astype(np.float32)
        on += np.isin(pts[a], bounds).sum()
        below += np.isin(pts[a], np.nextafter(bounds, np.float32(-np.inf))).sum()
        above += np.isin(pts[a], np.nextafter(bounds, np.float32(np.inf))).sum()
    assert (on, below, above) == (12, 12, 12)
    q32 = (pts - origin[:, None]).astype(np.float32) / np.float32(v)        # the fp32 difference puts some back ON it
    assert (q32 == np.round(q32)).sum() > on
    pts, v, origin, dims = PE.voxel_clamp_scene()
    idx = np.floor((pts - origin[:, None]) / np.float32(v))
    for a in range(3):
        assert (idx[a] < 0).any() and (idx[a] >= dims[a]).any() and ((idx[a] >= 0) & (idx[a] < dims[a])).any()
    assert PE.voxel_ref(pts, v, origin, dims).shape[1] <= int(np.prod(dims))


# --------------------------------------------------------------------------------------------------------- crop scenes
def test_crop_scenes_keep_what_they_say():
    for n in PE.CROP_N:
        for pattern in PE.CROP_PATTERNS:
            pts, keep = PE.crop_scene(n, pattern)
            assert pts.shape == (3, n)
            assert np.array_equal(OP.filter_work_space(pts, PE.CROP_BOX), np.nonzero(keep)[0])
    assert PE.crop_keep(3073, "lane63").sum() == 48 and PE.crop_keep(3073, "thread0").sum() == 4
    pts = PE.crop_nonfinite_scene()
    bad = ~np.isfinite(pts).all(axis=0)
    assert bad.sum() == 27 and np.array_equal(OP.filter_work_space(pts, PE.CROP_BOX), np.nonzero(~bad)[0])
    for a in range(3):
        assert np.isnan(pts[a]).sum() == 3 and np.isposinf(pts[a]).sum() == 3 and np.isneginf(pts[a]).sum() == 3
    pts, inside = PE.crop_faces_scene()
    assert inside.sum() == 6 and np.array_equal(OP.filter_work_space(pts, PE.CROP_BOX), np.nonzero(inside)[0])
    for box in PE.CROP_EMPTY_BOXES:
        assert len(OP.filter_work_space(PE.crop_scene(1025, "all")[0], box)) == 0


# --------------------------------------------------------------------------------------------------------- the wrapper's grid
def test_voxel_grid_helper_equals_the_oracle_on_finite_input():
    from s4g_release_amd.preprocess import _voxel_grid
    clouds = [(PE.tabletop(500), 0.005), (PE.tabletop(4000), 0.013), PE.voxel_bounds_scene()]
    clouds += [PE.voxel_bits_scene(k)[:2] for k in range(len(PE.BITS_LADDER))]
    for pts, v in clouds:
        origin, dims = _voxel_grid(pts.min(axis=1), pts.max(axis=1), v)
        want_o, want_d = OP.voxel_grid(pts, v)
        assert origin.dtype == np.float32 and origin.tobytes() == want_o.tobytes()
        assert [int(x) for x in dims] == [int(x) for x in want_d]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_voxel_grid_helper_refuses_non_finite_bounds(axis, bad):
    from s4g_release_amd.preprocess import _voxel_grid
    pts = PE.tabletop(100)
    lo, hi = pts.min(axis=1), pts.max(axis=1)
    for which in ("lo", "hi"):
        l, h = lo.copy(), hi.copy()
        (l if which == "lo" else h)[axis] = bad
        with pytest.raises(RuntimeError, match="non-finite coordinates.*crop first"):
            _voxel_grid(l, h, 0.005)


def test_voxel_grid_helper_refuses_grids_the_kernel_cannot_index():
    from s4g_release_amd.preprocess import _voxel_grid
    lo = np.zeros(3, np.float32)
    with pytest.raises(RuntimeError, match="too fine"):                      # one axis of 2^31 cells or more
        _voxel_grid(lo, np.array([2.0 ** 31, 0, 0], np.float32), 1.0)
    with pytest.raises(RuntimeError, match="too fine"):                      # 2^32 cells in all
        _voxel_grid(lo, np.array([65535.0, 65535.0, 0], np.float32), 1.0)
    with pytest.raises(RuntimeError, match="too fine"):                      # the quotient overflows fp32
        _voxel_grid(lo, np.array([1e30, 0, 0], np.float32), 1e-30)
    origin, dims = _voxel_grid(lo, np.array([65535.0, 65534.0, 0], np.float32), 1.0)
    assert [int(x) for x in dims] == [65536, 65535, 1]                        # the largest grid that is served
