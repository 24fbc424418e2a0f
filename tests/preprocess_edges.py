"""The edges of the pre-processing kernels (csrc/preprocess.hip): crop, voxel down-sample, radius-outlier removal.
Plain data, seeded constructions and two reference functions.  tests/test_preprocess_edges.py keeps the table honest
on the CPU (the constants against the sources, the references against oracle/preprocess.py, every construction
against what it is there for); tests/test_preprocess_edges_gpu.py runs every scene on the device, bit for bit.

What the scenes are built around:
  radius   `s4g_radius_outlier_mask_f32` bins the cloud into the ball query's toroidal 32^3 cell grid (csrc/grid.h;
           cell edge = radius (1 + 1/256), origin = point 0) and counts, per point, the records of three x-runs in
           each of nine (y, z) rows; a run that crosses x = 31 -> 0 is read as two.  A scene with a point more than
           GR_COORD_LIMIT - 1 cells from point 0 (or a NaN / inf coordinate) is flagged and every thread scans the
           cloud; N > GR_MAX_POINTS or radius >= 1e18 takes `radius_count_scan_kernel` with no grid at all.  The
           build kernel has three forms, switched at 8 x 1 024 and 25 x 1 024 points.
  voxel    keys (iz dy + iy) dx + ix are uint32, sorted on `bits` = ceil(log2(cells)) bits, 8 per pass; heads,
           an exclusive scan and one thread per cell (double sum in point order) follow, in blocks of 256 and
           sort / scan tiles of 2 048.
  crop     one workgroup of 1 024 threads walks the cloud; a wave's ballot gives the rank inside the round.

The cell function below restates `grid_coord`; it is used ONLY to place points and to assert where they fell, never
to compute an expectation: `counts_ref` finds its candidates through a float64 hash with another cell edge.
"""
import functools
from fractions import Fraction

import numpy as np

# --------------------------------------------------------------------------------------------------------- constants
GR_DIM = 32                      # csrc/grid.h
GR_COORD_LIMIT = 4096
GR_MAX_POINTS = 65536
GR_BUILD_THREADS = 1024
GR_WIDEN = 1.0 / 256.0           # cell edge = radius (1 + GR_WIDEN), s4g_radius_outlier_mask_f32
GR_BUILD_LADDER = (8, 25)        # launch_grid_build: points per build thread up to which a register form runs
RADIUS_SCAN_FROM = 1e18          # radius at and above which no grid is built
PP_THREADS = 1024                # crop: points per round
VOXEL_THREADS = 256              # voxel key / head / mean kernels
SORT_TILE = 2048                 # keys per workgroup of the radix sort and the scan
WAVE = 64


def cell_edge(radius):
    """The grid's cell edge as the entry computes it (fp32)."""
    return np.float32(np.float32(radius) * np.float32(1.0 + GR_WIDEN))


def cell_coord(v, o, radius):
    """floor(fp32(fp32(v - o) inv_h)), inv_h = fp32(1 / cell_edge): grid_coord restated.  Float result (NaN, inf and
    values past int32 stay what they are).  For placing points and asserting where they fell only."""
    inv_h = np.float32(np.float32(1.0) / cell_edge(radius))
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(v, dtype=np.float32) - np.asarray(o, dtype=np.float32)).astype(np.float32)
        return np.floor((d * inv_h).astype(np.float32)).astype(np.float64)


def cells_of(points_3n, radius):
    """(3, N) cell coordinates of a scene relative to its point 0."""
    return np.stack([cell_coord(points_3n[a], points_3n[a, 0], radius) for a in range(3)])


def seed_of(*key):
    return int(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.flags.writeable = False
    return a


def tabletop(n, scene=7):
    from s4g_release_amd import synth
    return synth.make_batch([scene], n)[0]


# --------------------------------------------------------------------------------------------------------- counts_ref
def _round_f32(q):
    """The fp32 nearest to the rational q, ties to even: q is compared with the fp32 neighbours of its double."""
    f = np.float32(float(q))
    cands = sorted({float(np.nextafter(f, np.float32(-np.inf))), float(f), float(np.nextafter(f, np.float32(np.inf)))})
    below = max(c for c in cands if Fraction(c) <= q)
    above = min(c for c in cands if Fraction(c) >= q)
    if below == above:
        return np.float32(below)
    lo, hi = q - Fraction(below), Fraction(above) - q
    if lo != hi:
        return np.float32(below if lo < hi else above)
    return np.float32(below if (np.float32(below).view(np.uint32) & 1) == 0 else above)


def fmad_dist2_exact(dx, dy, dz):
    """dist2<true> of csrc/s4g_common.h for one pair of fp32 differences: t = dx dx; t = fma(dy, dy, t);
    t = fma(dz, dz, t), each fma rounded once (exact rational arithmetic)."""
    t = np.float32(np.float32(dx) * np.float32(dx))
    t = _round_f32(Fraction(float(dy)) * Fraction(float(dy)) + Fraction(float(t)))
    return _round_f32(Fraction(float(dz)) * Fraction(float(dz)) + Fraction(float(t)))


def _inside(p, i, j, r2, fmad):
    """Boolean per candidate pair: canonical squared distance of points i and j < r2 (fp32)."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = (p[0, j] - p[0, i]).astype(np.float32)
        dy = (p[1, j] - p[1, i]).astype(np.float32)
        dz = (p[2, j] - p[2, i]).astype(np.float32)
        if not fmad:
            d = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
            d = (d + (dz * dz).astype(np.float32)).astype(np.float32)
            return d < r2
        d64 = dx.astype(np.float64) ** 2 + dy.astype(np.float64) ** 2 + dz.astype(np.float64) ** 2
        if not np.isfinite(r2):
            return d64 < np.float64(r2)          # the fp32 result is finite wherever the float64 one is this small
        inside = d64 < np.float64(r2)
        near = np.nonzero(np.abs(d64 - np.float64(r2)) <= 2.0 ** -20 * np.float64(r2))[0]
        for k in near:                            # the fp32 result is within 2^-22 r2 of d64: only these can differ
            inside[k] = fmad_dist2_exact(dx[k], dy[k], dz[k]) < r2
        return inside


def counts_ref(points_3n, radius, fmad=False):
    """Number of points (the point itself included) at canonical fp32 squared distance < fp32(r) fp32(r):
    ((dx dx + dy dy) + dz dz), or with fmad the fused form.  A pair with a NaN (or inf) coordinate never counts, the
    point itself included.  Candidates: a float64 cell hash with cell edge 1.01 r over the 27 surrounding cells;
    where that hash cannot be formed (cell indices past 2^62: a denormal r^2) every pair is a candidate."""
    p = np.asarray(points_3n, dtype=np.float32)
    n = p.shape[1]
    with np.errstate(over="ignore", under="ignore"):
        r2 = np.float32(radius) * np.float32(radius)
    cnt = np.zeros(n, dtype=np.int64)
    fin = np.nonzero(np.isfinite(p).all(axis=0))[0]
    if len(fin) == 0:
        return cnt
    edge = 1.01 * float(np.float32(radius))
    with np.errstate(over="ignore"):
        c = np.floor(p[:, fin].astype(np.float64) / edge)
    hashed = np.isfinite(c).all() and np.abs(c).max() < 2.0 ** 40
    if hashed:
        c = c.astype(np.int64)
        c -= c.min(axis=1, keepdims=True) - 1                     # 1 .. extent: the padding keeps rows apart
        ext = [int(e) + 2 for e in c.max(axis=1)]
        hashed = ext[0] * ext[1] * ext[2] < 2 ** 62
    if not hashed:
        assert len(fin) <= 4096, "all-pairs fallback is for small scenes"
        i, j = np.meshgrid(fin, fin, indexing="ij")
        i, j = i.ravel(), j.ravel()
        np.add.at(cnt, i[_inside(p, i, j, r2, fmad)], 1)
        return cnt
    key = (c[2] * ext[1] + c[1]) * ext[0] + c[0]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    uk, start, size = np.unique(ks, return_index=True, return_counts=True)
    cell_of = np.searchsorted(uk, ks)                             # cell number of every sorted point
    m = len(ks)
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                nk = uk + (oz * ext[1] + oy) * ext[0] + ox
                pos = np.minimum(np.searchsorted(uk, nk), len(uk) - 1)
                have = uk[pos] == nk
                s = np.where(have, start[pos], 0)[cell_of]        # per sorted point: its neighbour cell's run
                k = np.where(have, size[pos], 0)[cell_of]
                total = int(k.sum())
                if total == 0:
                    continue
                first = np.cumsum(k) - k
                a = np.repeat(np.arange(m), k)
                b = np.repeat(s, k) + (np.arange(total) - np.repeat(first, k))
                i, j = fin[order[a]], fin[order[b]]
                cnt += np.bincount(i[_inside(p, i, j, r2, fmad)], minlength=n)
    return cnt


# --------------------------------------------------------------------------------------------------------- voxel_ref
def voxel_ref(points_3n, voxel, origin, dims):
    """oracle.preprocess.voxel_down_sample over a GIVEN grid: cell = clip(floor(fp32(fp32(p - origin) / voxel)),
    0, dims - 1), cells ascending in (iz, iy, ix), mean = double sum in point order, one rounding."""
    p = np.asarray(points_3n, dtype=np.float32)
    if p.shape[1] == 0:
        return p.copy()
    v = np.float32(voxel)
    o = np.asarray(origin, dtype=np.float32).reshape(3, 1)
    d = np.asarray(dims, dtype=np.int64).reshape(3, 1)
    idx = np.floor(((p - o).astype(np.float32) / v).astype(np.float32)).astype(np.int64)
    idx = np.clip(idx, 0, d - 1)
    key = (idx[2] * int(d[1, 0]) + idx[1]) * int(d[0, 0]) + idx[0]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    heads = np.nonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))[0]
    ends = np.concatenate([heads[1:], [len(ks)]])
    out = np.empty((3, len(heads)), dtype=np.float32)
    p64 = p.astype(np.float64)
    for c, (a, b) in enumerate(zip(heads, ends)):
        s = np.zeros(3, dtype=np.float64)
        for j in order[a:b]:
            s += p64[:, j]
        out[:, c] = (s / float(b - a)).astype(np.float32)
    return out


def key_bits(dims):
    """The key width `s4g_voxel_down_sample_f32` sorts on."""
    cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    bits = 1
    while bits < 32 and (1 << bits) < cells:
        bits += 1
    return bits


# ===================================================================================================== radius scenes
class Scene:
    """points (3, N) float32 (read-only), radius, and whatever the construction wants checked."""

    def __init__(self, name, points, radius, **meta):
        self.name, self.points, self.radius = name, _frozen(np.asarray(points, dtype=np.float32)), float(radius)
        self.n = self.points.shape[1]
        self.__dict__.update(meta)

    @functools.lru_cache(maxsize=None)
    def counts(self, fmad=False):
        return _frozen(counts_ref(self.points, self.radius, fmad))


# ---- the size ladder: the launch block (256), the build kernel's switches (8 x 1 024, 25 x 1 024), grid / scan
# (GR_MAX_POINTS).  Radius and nb per size: table-top clouds are surfaces, so the neighbour count goes with N r^2;
# with nb = 4, N r^2 = 1.64 (r = 0.005 at 65 537 points) keeps 86 % there, 1.2 about 80 % of the middle sizes and
# 0.7 about 60 % of the small ones (kept shares: profiles/r24_preprocess_edges.md).  One and two points cannot be split
# (a single point keeps itself or not; two points see each other or not, both alike): those rows run at both outcomes
# instead.
RADIUS_LADDER_N = [1, 2, 255, 256, 257, 8192, 8193, 25600, 25601, 65535, 65536, 65537]
LADDER_NB = 4


def ladder_radius(n):
    if n >= 65535:
        return 0.005
    return float(np.float32(np.sqrt((1.2 if n >= 8192 else 0.7) / max(n, 255))))


@functools.lru_cache(maxsize=None)
def ladder_scene(n):
    return Scene("ladder%d" % n, tabletop(n), ladder_radius(n))


def ladder_nbs(n):
    """The thresholds a ladder row runs at."""
    return [0, n] if n <= 2 else [LADDER_NB]


# ---- the torus scene
TORUS_RADIUS = 0.02
TORUS_NB = 6
TORUS_ORIGIN = (0.3125, -0.1875, 0.875)
TORUS_REACH = 40                                  # lattice cells to both sides of point 0
TORUS_X_CELLS = (-2, -1, 0, 1, 30, 31, 32, 33)    # = 30, 31, 0, 1 (mod 32), below and above zero
TORUS_CORE_SIZES = (TORUS_NB - 2, TORUS_NB - 1, TORUS_NB, TORUS_NB + 1)


@functools.lru_cache(maxsize=None)
def torus_scene():
    """Point 0 (the grid origin) in the middle of a sparse lattice that reaches TORUS_REACH cells to both sides on every
    axis: the three axis lines, one point per cell centre, and seeded points sprinkled through the cube -- 81 cells
    across a 32-cell torus, so every cell shares its slot with cells 32 and 64 away.

    Clusters: `core` points within 0.25 r of a cell centre (|dx| <= 0.05 r) and two probes 0.9 r off the centre along
    -x and +x, which lie in the x-neighbour cells and within r of every core point.  A core point therefore counts
    core + 2 points, a probe core + 1; with core in nb - 2 .. nb + 1 both kinds land on nb and on nb + 1.  The cluster
    cells have x = 30, 31, 0, 1 (mod 32): the run (x - 1 .. x + 1) of a core point or a probe crosses 31 -> 0 in
    every way, and a probe's cluster lies in the first run for one and in the second run for another.  Every cluster
    is repeated exactly 32 cells away along x, along y and along z (same slot, 32 cells apart: must not be counted).
    """
    r, h = TORUS_RADIUS, float(cell_edge(TORUS_RADIUS))
    o = np.array(TORUS_ORIGIN, dtype=np.float64)
    rng = np.random.default_rng(seed_of(32, 3))
    pts, kind, cell, alias_of, shift_axis = [o.copy()], ["origin"], [(0, 0, 0)], [-1], [-1]

    def put(c, off, k, base=-1, axis=-1):
        pts.append(o + (np.array(c, dtype=np.float64) + 0.5) * h + off)
        kind.append(k)
        cell.append(tuple(int(v) for v in c))
        alias_of.append(base)
        shift_axis.append(axis)
        return len(pts) - 1

    rows = [(y, z) for y in (-12, -8, -4, 4, 8, 12) for z in (-12, -8, -4, 4, 8, 12)]
    taken = set()
    k = 0
    for x in TORUS_X_CELLS:
        for core in TORUS_CORE_SIZES:
            y, z = rows[k]
            k += 1
            offs = []
            for _ in range(core):
                d = rng.standard_normal(3)
                d *= 0.25 * r * rng.random() ** (1.0 / 3.0) / np.linalg.norm(d)
                d[0] = np.clip(d[0], -0.05 * r, 0.05 * r)
                offs.append(d)
            members = [((x, y, z), d, "core") for d in offs]
            # the probes: centre -+ 0.9 r in x, written relative to the centre of the neighbour cell they fall in
            members.append(((x - 1, y, z), np.array([h - 0.9 * r, 0.0, 0.0]), "probe-"))
            members.append(((x + 1, y, z), np.array([0.9 * r - h, 0.0, 0.0]), "probe+"))
            base_idx = [put(c, d, kd) for c, d, kd in members]
            for axis in range(3):
                for (c, d, kd), bi in zip(members, base_idx):
                    ca = list(c)
                    ca[axis] += GR_DIM
                    put(ca, d, kd, bi, axis)
            for dx in range(-4, 5):
                for dy in range(-3, 4):
                    for dz in range(-3, 4):
                        for sx, sy, sz in ((0, 0, 0), (GR_DIM, 0, 0), (0, GR_DIM, 0), (0, 0, GR_DIM)):
                            taken.add((x + dx + sx, y + dy + sy, z + dz + sz))
    for axis in range(3):
        for v in range(-TORUS_REACH, TORUS_REACH + 1):
            c = [0, 0, 0]
            c[axis] = v
            put(c, np.zeros(3), "lattice")
    n_sprinkle = 0
    while n_sprinkle < 1700:
        c = tuple(int(v) for v in rng.integers(-TORUS_REACH, TORUS_REACH + 1, size=3))
        if c in taken:
            continue
        put(c, (rng.random(3) - 0.5) * 0.9 * h, "sprinkle")
        n_sprinkle += 1
    return Scene("torus", np.array(pts).T.astype(np.float32), r, nb=TORUS_NB, kind=np.array(kind),
                 cell=np.array(cell).T, alias_of=np.array(alias_of), shift_axis=np.array(shift_axis))


# ---- the 27-cell scene
CELL27_RADIUS = 0.02
CELL27_CENTRES = {"positive": (5, 5, 5), "negative": (-7, -9, -4), "wrap": (31, 0, -1)}


def cell27_offsets():
    """The 26 partner offsets in units of r: +-0.9 along an axis, +-0.65 on two axes, +-0.55 on all three (norms
    0.9, 0.92, 0.95: all inside r; every component beyond half a cell: all in a neighbour cell)."""
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nz = abs(dx) + abs(dy) + abs(dz)
                if nz:
                    out.append(np.array([dx, dy, dz], dtype=np.float64) * {1: 0.9, 2: 0.65, 3: 0.55}[nz])
    return out


@functools.lru_cache(maxsize=None)
def cell27_scene(which):
    """Point 0 (the origin, alone), the centre point at the middle of cell CELL27_CENTRES[which], then 26 partners."""
    r, h = CELL27_RADIUS, float(cell_edge(CELL27_RADIUS))
    o = np.array(TORUS_ORIGIN, dtype=np.float64)
    centre = o + (np.array(CELL27_CENTRES[which], dtype=np.float64) + 0.5) * h
    pts = [o, centre] + [centre + r * d for d in cell27_offsets()]
    return Scene("cell27-" + which, np.array(pts).T.astype(np.float32), r, centre_cell=CELL27_CENTRES[which])


# ---- the pair scene
PAIR_RADIUS = 0.02
PAIR_COUNT = 2048
PAIR_SEED = 1


@functools.lru_cache(maxsize=None)
def pair_scene(seed=PAIR_SEED):
    """PAIR_COUNT isolated pairs on a 0.1-spaced 16 x 16 x 8 lattice (80 cells across: aliased slots again): point
    2 k is the lattice point a, point 2 k + 1 is fp32(a + r u), u a seeded unit vector.  The rounding of the three
    coordinates puts the pair's fp32 squared distance below, at, or above fp32(r)^2; with nb = 1 both points are kept
    iff it is below."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(8), indexing="ij")).reshape(3, -1)
    a = (g * 0.1).astype(np.float32)
    u = rng.standard_normal((3, PAIR_COUNT))
    u /= np.linalg.norm(u, axis=0)
    b = (a.astype(np.float64) + PAIR_RADIUS * u).astype(np.float32)
    pts = np.empty((3, 2 * PAIR_COUNT), dtype=np.float32)
    pts[:, 0::2], pts[:, 1::2] = a, b
    return Scene("pairs", pts, PAIR_RADIUS, nb=1)


def pair_dist2(scene, fmad=False):
    """fp32 squared distance of every pair under the contract (fmad: the exact fused form)."""
    p = scene.points
    d = (p[:, 1::2] - p[:, 0::2]).astype(np.float32)
    if fmad:
        return np.array([fmad_dist2_exact(*d[:, k]) for k in range(d.shape[1])], dtype=np.float32)
    return ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pair_variant_scene(which):
    """The pair scene through the other two loops that compare against r^2: "flier" adds one point FLIER_CELLS cells
    from point 0 (the scene is flagged: the scan branch of radius_count_kernel), "scan" adds a table-top cloud 10 m away
    up to GR_MAX_POINTS + 1 points (radius_count_scan_kernel)."""
    base = pair_scene()
    if which == "flier":
        extra = base.points[:, :1].copy()
        extra[0, 0] = np.float32(np.float64(extra[0, 0]) + (FLIER_CELLS + 0.5) * float(cell_edge(base.radius)))
    else:
        assert which == "scan"
        extra = tabletop(GR_MAX_POINTS + 1 - base.n, scene=5)
        extra[0] += np.float32(10.0)
    return Scene("pairs-" + which, np.concatenate([base.points, extra], axis=1), base.radius, nb=1)


# ---- the fallback scenes: anything that sets the scene's flag sends every thread through the scan branch
FLIER_CELLS = 5000


@functools.lru_cache(maxsize=None)
def fallback_scene(which):
    base = torus_scene()
    p = np.concatenate([base.points, np.zeros((3, 1), np.float32)], axis=1)
    p[:, -1] = p[:, 0]
    p[0, -1] = np.float32(np.float64(p[0, 0]) + (FLIER_CELLS + 0.5) * float(cell_edge(base.radius)))
    if which == "nan-origin":
        p[0, 0] = np.nan
    elif which == "nan-later":
        p[1, 1234] = np.nan
    elif which == "inf-later":
        p[2, 77] = np.inf
        p[0, 78] = -np.inf
    elif which == "nan-only":                   # no flier: the NaN point alone flags the scene
        p = p[:, :-1].copy()
        p[2, 2000] = np.nan
    else:
        assert which == "flier"
    return Scene("fallback-" + which, p, base.radius, nb=base.nb)


FALLBACK_KINDS = ("flier", "nan-origin", "nan-later", "inf-later", "nan-only")


# ---- degenerate parameters: (name, scene, [nb])
@functools.lru_cache(maxsize=None)
def degenerate_cases():
    cloud = tabletop(300)
    n = cloud.shape[1]
    nan_cloud = cloud.copy()
    nan_cloud[1, 17] = np.nan
    # duplicate groups of 1, 2 and 3 points, interleaved; point 0 belongs to a group of 3
    a, b, c, d = cloud[:, 0], cloud[:, 1], cloud[:, 2], cloud[:, 3]
    dups = np.stack([a, b, c, a, d, c, a, cloud[:, 4], cloud[:, 5], d, cloud[:, 6], c], axis=1)
    group = np.array([3, 1, 3, 3, 2, 3, 3, 1, 1, 2, 1, 3])
    same = np.repeat(cloud[:, 9:10], 5, axis=1)                   # one cell, no flag: the grid branch
    nbs = [0, n - 1, n, 2 ** 31 - 1]
    return (
        # radius >= 1e18: the scan kernel; fp32(1e19)^2 = 1e38 is finite, fp32(1e20)^2 is inf: every finite point
        # counts under both
        ("r1e19", Scene("r1e19", cloud, 1e19), nbs),
        ("r1e20", Scene("r1e20", cloud, 1e20), [n - 1, n]),
        ("r1e19-nan", Scene("r1e19-nan", nan_cloud, 1e19), [n - 2, n - 1]),
        # the same thresholds through the grid
        ("grid-nb", Scene("grid-nb", cloud, 0.05), nbs),
        ("r1-all", Scene("r1-all", cloud, 1.0), [n - 1, n]),
        # r^2 = 1e-40 is an fp32 denormal: only exact duplicates (distance 0) count
        ("r1e-20", Scene("r1e-20", dups, 1e-20, group=group), [0, 1, 2, 3]),
        ("r1e-20-one-cell", Scene("r1e-20-one-cell", same, 1e-20), [4, 5]),
        # r^2 = 0: 0 < 0 is false, nothing counts, not even the point itself
        ("r1e-23", Scene("r1e-23", dups, 1e-23), [0]),
        ("r1e-23-one-cell", Scene("r1e-23-one-cell", same, 1e-23), [0]),
    )


def radius_cases():
    """[(id, scene getter, nb)] -- every radius scene with every threshold it runs at."""
    out = []
    for n in RADIUS_LADDER_N:
        for nb in ladder_nbs(n):
            out.append(("ladder%d-nb%d" % (n, nb), functools.partial(ladder_scene, n), nb))
    out.append(("torus", torus_scene, TORUS_NB))
    for which in CELL27_CENTRES:
        for nb in (26, 27):
            out.append(("cell27-%s-nb%d" % (which, nb), functools.partial(cell27_scene, which), nb))
    out.append(("pairs", pair_scene, 1))
    for which in ("flier", "scan"):
        out.append(("pairs-" + which, functools.partial(pair_variant_scene, which), 1))
    for which in FALLBACK_KINDS:
        out.append(("fallback-" + which, functools.partial(fallback_scene, which), TORUS_NB))
    for i, (name, _, nbs) in enumerate(degenerate_cases()):
        for nb in nbs:
            out.append(("%s-nb%d" % (name, nb), functools.partial(lambda k: degenerate_cases()[k][1], i), nb))
    return out


FMAD_CASES = ("pairs", "pairs-flier", "pairs-scan", "torus", "ladder65537-nb%d" % LADDER_NB)
TWICE_CASE = "ladder8193-nb%d" % LADDER_NB


# ====================================================================================================== voxel scenes
VOXEL_N = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4097]
VOXEL_FILLS = ("own-cell", "one-cell", "mix")
VOXEL_EDGE = 2.0 ** -7
VOXEL_BASE = (0.25, -1.5, 0.75)                   # multiples of the edge: every cell centre is exact in fp32
MIX_PATTERN = (300, 1, 2, 2, 1, 1, 2)


@functools.lru_cache(maxsize=None)
def voxel_fill_scene(n, fill):
    """(points (3, n), voxel).  Cell centres are base + c voxel (the wrapper's origin is min - voxel / 2).
    own-cell: n distinct cells in shuffled order, both corners of their box among them;
    one-cell: n points inside the lower half of one cell (above the minimum, which is the cell's centre);
    mix: cells of 300 / 1 / 2 / ... points in shuffled order, offsets inside a cell +- voxel/4 2^-u, u in [0, 12], so
         an fp32 sum loses bits the double sum keeps; the first cell sits around the coordinate zero and holds
         magnitudes down to 2^-40 of either sign, which a double sum in another order rounds differently."""
    rng = np.random.default_rng(seed_of(n, VOXEL_FILLS.index(fill), 11))
    v = VOXEL_EDGE
    base = np.array(VOXEL_BASE, dtype=np.float64).reshape(3, 1)
    if fill == "own-cell":
        side = int(np.ceil((2.0 * n) ** (1.0 / 3.0))) + 1
        flat = rng.choice(side ** 3 - 2, size=max(n - 2, 0), replace=False) + 1
        flat = np.concatenate([[0], flat, [side ** 3 - 1]])[:n] if n > 1 else np.array([0])
        c = np.stack(np.unravel_index(rng.permutation(flat), (side, side, side))).astype(np.float64)
        pts = base + c * v
    elif fill == "one-cell":
        pts = base + rng.random((3, n)) * 0.49 * v
        pts[:, n // 2] = base[:, 0]
    else:
        cells, left, k = [], n, 0
        while left:
            s = min(MIX_PATTERN[k % len(MIX_PATTERN)], left)
            cells.append(s)
            left -= s
            k += 1
        side = int(np.ceil(len(cells) ** (1.0 / 3.0))) + 1
        where = rng.choice(side ** 3, size=len(cells), replace=False)
        cols = []
        for ci, s in enumerate(cells):
            # cells 1 .. side on every axis: nothing but the first cell's minimum reaches down to cell 0's centre
            c = np.array(np.unravel_index(where[ci], (side, side, side)), dtype=np.float64).reshape(3, 1) + 1.0
            if ci == 0:
                # base is moved to -voxel/4 below: cell 0 is [-3/4, 1/4) voxel and holds zero
                off = rng.choice([-1.0, 1.0], size=(3, s)) * 0.24 * v * 2.0 ** -rng.uniform(0, 40, size=(3, s))
                off[:, 0] = -0.25 * v                             # the cloud's minimum: the cell's centre
                cols.append(off)
            else:
                off = rng.choice([-1.0, 1.0], size=(3, s)) * 0.25 * v * 2.0 ** -rng.uniform(0, 12, size=(3, s))
                cols.append(-0.25 * v + c * v + off)
        pts = np.concatenate(cols, axis=1)[:, rng.permutation(n)]
    return _frozen(pts.astype(np.float32)), v


# total cells -> (dims, voxel, bits)
BITS_LADDER = [
    ((1, 1, 1), 2.0 ** -7, 1),
    ((2, 1, 1), 2.0 ** -7, 1),
    ((15, 17, 1), 2.0 ** -7, 8),
    ((4, 8, 8), 2.0 ** -7, 8),
    ((257, 1, 1), 2.0 ** -7, 9),
    ((64, 32, 32), 2.0 ** -7, 16),
    ((65537, 1, 1), 2.0 ** -10, 17),
    ((256, 256, 256), 2.0 ** -7, 24),
    ((97, 257, 673), 2.0 ** -7, 25),
    ((65536, 65535, 1), 2.0 ** -10, 32),
]
BITS_CELLS = [1, 2, 255, 256, 257, 65536, 65537, 2 ** 24, 2 ** 24 + 1, 65536 * 65535]


@functools.lru_cache(maxsize=None)
def voxel_bits_scene(k):
    """(points, voxel, dims): 48 points in shuffled order over a grid of BITS_LADDER[k] cells -- its eight corners,
    seeded cells (the upper half of the key range among them), and every fourth cell twice."""
    dims, v, _ = BITS_LADDER[k]
    rng = np.random.default_rng(seed_of(k, 23))
    d = np.array(dims)
    corners = np.array([[x, y, z] for z in (0, d[2] - 1) for y in (0, d[1] - 1) for x in (0, d[0] - 1)])
    rand = np.stack([rng.integers(0, d[a], size=28) for a in range(3)], axis=1)
    top = np.stack([rng.integers(0, d[0], size=4), rng.integers(d[1] // 2, d[1], size=4),
                    rng.integers(d[2] // 2, d[2], size=4)], axis=1)
    c = np.concatenate([corners, rand, top])
    c = np.concatenate([c, c[::4][:8]])[rng.permutation(48)]
    base = np.array([-16.0, 2.0, 0.5]).reshape(3, 1)
    return _frozen((base + c.T.astype(np.float64) * v).astype(np.float32)), v, dims


@functools.lru_cache(maxsize=None)
def voxel_bounds_scene():
    """voxel 0.25, origin (1, -1, 0) exactly: per axis, points ON the cell bounds origin + k / 4, one ulp below and one
    ulp above, the other two coordinates at cell centres."""
    v = 0.25
    lo = np.array([1.125, -0.875, 0.125], dtype=np.float32)       # the minimum: origin + voxel / 2
    cols = [lo, lo + np.float32(1.0)]
    for axis in range(3):
        for k in (1, 2, 3, 4):
            edge = np.float32(lo[axis] - np.float32(0.125) + np.float32(0.25 * k))
            for val in (np.nextafter(edge, np.float32(-np.inf)), edge, np.nextafter(edge, np.float32(np.inf))):
                p = lo + np.float32(0.25) * np.float32((k + axis) % 3)
                p[axis] = val
                cols.append(p.astype(np.float32))
    return _frozen(np.stack(cols, axis=1).astype(np.float32)), v


@functools.lru_cache(maxsize=None)
def voxel_clamp_scene():
    """(points, voxel, origin, dims) for the C ABI: the grid is a box INSIDE the cloud, points outside it clamp into
    its border cells."""
    rng = np.random.default_rng(seed_of(5, 29))
    pts = (rng.integers(0, 4 * 64, size=(3, 600)) / 64.0).astype(np.float32)       # [0, 4) on a 2^-6 lattice
    return _frozen(pts), 0.25, np.array([1.0, 1.0, 1.0], np.float32), np.array([6, 5, 4], np.int32)


# ======================================================================================================= crop scenes
CROP_N = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
CROP_PATTERNS = ("all", "none", "lane63", "thread0", "alternating", "random")
CROP_BOX = (-0.5, 0.75, -1.0, 0.25, 0.125, 2.0)


def crop_keep(n, pattern):
    j = np.arange(n)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "lane63":
        return j % WAVE == WAVE - 1
    if pattern == "thread0":
        return j % PP_THREADS == 0
    if pattern == "alternating":
        return j % 2 == 1
    return np.random.default_rng(seed_of(n, 31)).random(n) < 0.37


@functools.lru_cache(maxsize=None)
def crop_scene(n, pattern):
    """(points (3, n), intended keep mask): kept points lie inside CROP_BOX, the others outside it on one seeded axis
    and side."""
    rng = np.random.default_rng(seed_of(n, CROP_PATTERNS.index(pattern), 37))
    lo, hi = np.array(CROP_BOX[0::2]).reshape(3, 1), np.array(CROP_BOX[1::2]).reshape(3, 1)
    keep = crop_keep(n, pattern)
    pts = lo + (hi - lo) * (0.01 + 0.98 * rng.random((3, n)))
    axis, side = rng.integers(0, 3, size=n), rng.integers(0, 2, size=n)
    out = np.where(side == 0, lo[axis, 0] - rng.random(n), hi[axis, 0] + rng.random(n))
    for a in range(3):
        sel = ~keep & (axis == a)
        pts[a, sel] = out[sel]
    return _frozen(pts.astype(np.float32)), keep


@functools.lru_cache(maxsize=None)
def crop_nonfinite_scene():
    """Inside points, every third one with NaN, +inf or -inf on one axis."""
    pts = crop_scene(90, "all")[0].copy()
    bad = [np.nan, np.inf, -np.inf]
    for k in range(27):
        pts[k % 3, 3 * k + 1] = bad[(k // 3) % 3]
    return _frozen(pts)


@functools.lru_cache(maxsize=None)
def crop_faces_scene():
    """Per face of CROP_BOX: a point on the face, one ulp inside, one ulp outside (the other coordinates inside)."""
    box = np.array(CROP_BOX, dtype=np.float32)
    mid = ((box[0::2] + box[1::2]) * np.float32(0.5)).astype(np.float32)
    cols, inside = [], []
    for axis in range(3):
        for face, inward in ((box[2 * axis], np.inf), (box[2 * axis + 1], -np.inf)):
            for val, ok in ((face, False), (np.nextafter(face, np.float32(inward)), True),
                            (np.nextafter(face, np.float32(-inward)), False)):
                p = mid.copy()
                p[axis] = val
                cols.append(p)
                inside.append(ok)
    return _frozen(np.stack(cols, axis=1)), np.array(inside)


CROP_EMPTY_BOXES = [
    (0.75, -0.5, -1.0, 0.25, 0.125, 2.0),         # inverted on x
    (-0.5, 0.75, 0.25, 0.25, 0.125, 2.0),         # empty on y (lo == hi)
    (-0.5, 0.75, -1.0, 0.25, 2.0, 0.125),         # inverted on z
]
