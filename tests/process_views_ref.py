"""A numpy yardstick for `process_views` (csrc/process_views.hip), written from its semantics, and the scenes both test
files run.  tests/test_process_views_ref.py keeps it honest on the CPU (its stages against oracle/preprocess.py, eight
sabotaged restatements against the constructions, the constants against the sources); tests/test_process_views_gpu.py
compares the device with it bit for bit.

Semantics, per view:
  crop    keep p iff lo < p < hi strictly on every axis, among the first `count` rows; order kept;
  voxel   cell = floor(fp32(fp32(p - origin) / voxel)) on the CALLER's grid (origin = min_bound - voxel / 2, dims =
          floor((max_bound - origin) / voxel) + 1, fp32); cells ascending in (iz, iy, ix); mean = double sum in index
          order, one rounding; trace = the highest ORIGINAL index in the cell;
  radius  keep a mean iff the number of means (itself included) at canonical fp32 squared distance < fp32(r) fp32(r)
          exceeds nb;
  output  the kept means in cell order and their traces, NaN / -1 behind them, and the three counts.
The neighbour counts are all pairs, in this file's own arithmetic (`tests.preprocess_edges._inside`): no cell grid.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import preprocess_edges as PE

Config = namedtuple("Config", "workspace voxel_size voxel_bounds nb_points radius")

# data_gen/configs/config.py:20-24 and the literals of processing_and_trace
# (data_gen/pcd_classes/torch_precomputed_single_view_point_cloud.py:88-89)
DATA_GEN = Config((-0.40, 0.40, -0.35, 0.35, 0.749, 1.2), 0.005, ((-0.5, -0.5, 0.7), (0.5, 0.5, 1.5)), 8, 0.04)

SABOTAGES = ("crop-non-strict", "trace-lowest", "trace-not-composed", "self-not-counted", "count-ge", "distance-le",
             "mean-fp32", "scene-base-dropped")


def voxel_grid(cfg):
    """(origin (3,) f32, dims (3,) int64): `_voxel_grid` of the package restated."""
    v = np.float32(cfg.voxel_size)
    lo = np.asarray(cfg.voxel_bounds[0], dtype=np.float32)
    hi = np.asarray(cfg.voxel_bounds[1], dtype=np.float32)
    origin = (lo - v * np.float32(0.5)).astype(np.float32)
    dims = np.floor(((hi - origin) / v).astype(np.float32)).astype(np.int64) + 1
    return origin, dims


def crop_ref(points_3n, live, workspace, sabotage=None):
    """Ascending indices (< live) of the rows strictly inside the box; NaN and inf fail every comparison."""
    p = np.asarray(points_3n, dtype=np.float32)[:, :live]
    w = np.asarray(workspace, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        if sabotage == "crop-non-strict":
            keep = (p[0] >= w[0]) & (p[0] <= w[1]) & (p[1] >= w[2]) & (p[1] <= w[3]) & (p[2] >= w[4]) & (p[2] <= w[5])
        else:
            keep = (p[0] > w[0]) & (p[0] < w[1]) & (p[1] > w[2]) & (p[1] < w[3]) & (p[2] > w[4]) & (p[2] < w[5])
    return np.nonzero(keep)[0].astype(np.int64)


def voxel_trace_ref(points_3m, voxel, origin, dims, sabotage=None):
    """(means (3, V) f32, trace (V,) int64 into the columns of points_3m), cells ascending."""
    p = np.asarray(points_3m, dtype=np.float32)
    if p.shape[1] == 0:
        return p.copy(), np.zeros(0, dtype=np.int64)
    v = np.float32(voxel)
    o = np.asarray(origin, dtype=np.float32).reshape(3, 1)
    d = np.asarray(dims, dtype=np.int64).reshape(3, 1)
    idx = np.floor(((p - o).astype(np.float32) / v).astype(np.float32)).astype(np.int64)
    idx = np.clip(idx, 0, d - 1)
    cell = (idx[2] * int(d[1, 0]) + idx[1]) * int(d[0, 0]) + idx[0]
    members = {}
    for j in range(p.shape[1]):                        # ascending index inside every cell
        members.setdefault(int(cell[j]), []).append(j)
    cells = sorted(members)
    means = np.empty((3, len(cells)), dtype=np.float32)
    trace = np.empty(len(cells), dtype=np.int64)
    for c, k in enumerate(cells):
        js = members[k]
        if sabotage == "mean-fp32":
            means[:, c] = p[:, js].mean(axis=1, dtype=np.float32)
        else:
            s = np.zeros(3, dtype=np.float64)
            for j in js:
                s += p[:, j].astype(np.float64)
            means[:, c] = (s / float(len(js))).astype(np.float32)
        trace[c] = js[0] if sabotage == "trace-lowest" else js[-1]
    return means, trace


def neighbour_counts(points_3v, radius, fmad=False, sabotage=None):
    """All pairs: the number of columns (the column itself included) at canonical fp32 squared distance < r^2."""
    p = np.asarray(points_3v, dtype=np.float32)
    n = p.shape[1]
    r2 = np.float32(radius) * np.float32(radius)
    cnt = np.zeros(n, dtype=np.int64)
    everyone = np.arange(n)
    for i in range(n):
        me = np.full(n, i)
        if sabotage == "distance-le":
            with np.errstate(over="ignore", invalid="ignore"):
                dx, dy, dz = [(p[a] - p[a, i]).astype(np.float32) for a in range(3)]
                d = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
                inside = (d + (dz * dz).astype(np.float32)).astype(np.float32) <= r2
        else:
            inside = PE._inside(p, me, everyone, r2, fmad)
        cnt[i] = int(inside.sum()) - (1 if sabotage == "self-not-counted" and inside[i] else 0)
    return cnt


def process_view_ref(points_3n, live, cfg, fmad=False, sabotage=None):
    """One view -> dict(points (3, K), index (K,), crop, voxel, count)."""
    p = np.asarray(points_3n, dtype=np.float32)
    live = int(min(max(live, 0), p.shape[1]))
    origin, dims = voxel_grid(cfg)
    kept = crop_ref(p, live, cfg.workspace, sabotage)
    means, trace = voxel_trace_ref(p[:, kept], np.float32(cfg.voxel_size), origin, dims, sabotage)
    cnt = neighbour_counts(means, cfg.radius, fmad, sabotage)
    ok = cnt >= cfg.nb_points if sabotage == "count-ge" else cnt > cfg.nb_points
    index = trace[ok] if sabotage == "trace-not-composed" else kept[trace[ok]]
    return dict(points=means[:, ok], index=index, crop=len(kept), voxel=means.shape[1], count=int(ok.sum()))


Result = namedtuple("Result", "points index_in_ref crop_count voxel_count count")


def process_views_ref(clouds_b3n, count, cfg, fmad=False, sabotage=None):
    """B views -> Result of padded arrays: points (B, 3, N) NaN-padded, index_in_ref (B, N) -1-padded, counts (B,)."""
    x = np.asarray(clouds_b3n, dtype=np.float32)
    B, _, N = x.shape
    points = np.full((B, 3, N), np.nan, dtype=np.float32)
    index = np.full((B, N), -1, dtype=np.int32)
    counts = np.zeros((3, B), dtype=np.int32)
    for b in range(B):
        src = x[0] if sabotage == "scene-base-dropped" else x[b]
        r = process_view_ref(src, N if count is None else int(count[b]), cfg, fmad, sabotage)
        k = r["count"]
        points[b, :, :k] = r["points"]
        index[b, :k] = r["index"]
        counts[:, b] = (r["crop"], r["voxel"], k)
    return Result(points, index, counts[0], counts[1], counts[2])


def same(a, b):
    """Bit for bit, field by field."""
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() and np.asarray(u).shape == np.asarray(v).shape
               for u, v in zip(a, b))


# ============================================================================================================ scenes
# The lattice configuration: voxel 2^-7 over the unit cube, so origin = -2^-8 and the cell faces (k - 1/2) 2^-7 are
# exact in fp32; radius 2^-5 = four cells; the crop box 1/16 inside the cube.
LATTICE = Config((0.0625, 0.9375, 0.0625, 0.9375, 0.0625, 0.9375), 2.0 ** -7, ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), 4,
                 2.0 ** -5)
CHUNK = Config((0.0625, 0.9375, 0.0625, 0.9375, 0.0625, 0.9375), 2.0 ** -9, ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), 1,
               2.0 ** -5)
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049]
V = 2.0 ** -7

Case = namedtuple("Case", "name clouds count cfg")


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.flags.writeable = False
    return a


def surface_view(n, seed, box=LATTICE.workspace):
    """(3, n): a dense patch (about one point per cell of 2^-7 and a half, random fp32 offsets: cells of several
    points, sums that fp32 rounds differently), every fifth point sprinkled through the whole box (isolated: the radius
    filter drops most), every seventh outside the box, and a NaN / +inf / -inf row each where n allows."""
    rng = np.random.default_rng(PE.seed_of(n, seed, 41))
    lo, hi = np.array(box[0::2]), np.array(box[1::2])
    side = min(0.8, 0.8 * V * np.sqrt(max(n, 1)))
    p = np.empty((3, n))
    p[0] = 0.5 + (rng.random(n) - 0.5) * side
    p[1] = 0.5 + (rng.random(n) - 0.5) * side
    p[2] = 0.5 + 0.25 * V * np.sin(40.0 * p[0]) + 0.01 * V * rng.random(n)
    j = np.arange(n)
    far = j % 5 == 3
    p[:, far] = (lo[:, None] + (hi - lo)[:, None] * rng.random((3, n)))[:, far]
    out = j % 7 == 2
    p[rng.integers(0, 3, n)[out], j[out]] = np.where(rng.random(int(out.sum())) < 0.5, -0.25, 1.25)
    p = p.astype(np.float32)
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        if n > 12 + 3 * k:
            p[k, 11 + 3 * k] = bad
    return p


@functools.lru_cache(maxsize=None)
def size_case(n):
    """Three views of n rows: all live, about half live, none live."""
    clouds = np.stack([surface_view(n, 1), surface_view(n, 2), surface_view(n, 3)])
    return Case("n%d" % n, _frozen(clouds), _frozen(np.array([n, n // 2 + 1 if n > 1 else 1, 0], np.int32)), LATTICE)


def _centre(c):
    """Centre of cell c (3,) of the lattice grid: c 2^-7 exactly."""
    return np.asarray(c, dtype=np.float64) * V


@functools.lru_cache(maxsize=None)
def constructions():
    rng = np.random.default_rng(PE.seed_of(9, 43))
    out = []
    n = 300
    # a live view, a view outside the box, a view with count 0 (its rows are live views' copies: never read)
    nothing = surface_view(n, 4).copy()
    nothing[2] = np.float32(1.5)
    out.append(Case("empty-scenes", np.stack([surface_view(n, 5), nothing, surface_view(n, 5)]),
                    np.array([n, n, 0], np.int32), LATTICE))
    # every row in one cell; nb = 0 keeps the single mean, whose trace is the last row
    one = (_centre((40, 41, 42))[:, None] + (rng.random((3, n)) - 0.5) * 0.98 * V).astype(np.float32)
    out.append(Case("one-cell", one[None], None, LATTICE._replace(nb_points=0)))
    # every row in its own cell, in shuffled order: a 17 x 18 patch of adjacent cells
    g = np.stack(np.meshgrid(np.arange(17), np.arange(18), indexing="ij")).reshape(2, -1)[:, :n]
    own = np.stack([g[0] + 30, g[1] + 30, np.full(g.shape[1], 64)]).astype(np.float64) * V
    own = own[:, rng.permutation(own.shape[1])].astype(np.float32)
    out.append(Case("own-cell", own[None], None, LATTICE))
    # exact duplicates: every row of a 60-row view five times, interleaved
    base = surface_view(60, 6)
    out.append(Case("duplicates", np.tile(base, (1, 5))[None], None, LATTICE))
    # rows that are not finite, one per axis and kind, between live rows; the rows past `count` are NaN
    bad = surface_view(n, 7).copy()
    for k, v in enumerate((np.nan, np.inf, -np.inf) * 3):
        bad[k // 3, 20 + 9 * k] = v
    bad[:, 250:] = np.nan
    out.append(Case("non-finite", bad[None], np.array([250], np.int32), LATTICE))
    # per face of the box: a row on it, one ulp inside, one ulp outside (the other coordinates inside); nb = 0
    box = np.array(LATTICE.workspace, dtype=np.float32)
    cols = []
    for axis in range(3):
        for face, inward in ((box[2 * axis], np.inf), (box[2 * axis + 1], -np.inf)):
            for val in (face, np.nextafter(face, np.float32(inward)), np.nextafter(face, np.float32(-inward))):
                p = np.array([0.3, 0.4, 0.6], dtype=np.float32) + np.float32(0.01) * np.float32(len(cols))
                p[axis] = val
                cols.append(p)
    out.append(Case("box-faces", np.stack(cols, axis=1)[None], None, LATTICE._replace(nb_points=0)))
    # rows ON the cell faces origin + k voxel = (k - 1/2) 2^-7, one ulp below and above; nb = 0
    cols = []
    for axis in range(3):
        for k in (20, 21, 22, 64):
            edge = np.float32((k - 0.5) * V)
            for val in (np.nextafter(edge, np.float32(-np.inf)), edge, np.nextafter(edge, np.float32(np.inf))):
                p = _centre((30 + 2 * axis, 50, 70)).astype(np.float32)
                p[axis] = val
                cols.append(p)
    out.append(Case("cell-faces", np.stack(cols, axis=1)[None], None, LATTICE._replace(nb_points=0)))
    # blocks of nb, nb + 1, nb - 1 and nb + 2 single-row cells, every cell of a block within two cells (r / 2) of the
    # others, the blocks 3 r apart: a mean counts exactly its block; only nb + 1 and nb + 2 exceed nb
    nb = LATTICE.nb_points
    blocks = []
    for which, size in enumerate((nb, nb + 1, nb - 1, nb + 2)):
        cells = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1)][:size]
        blocks += [_centre(np.array(c) + (20 + 12 * which, 24, 28)) for c in cells]   # blocks 12 cells = 3 r apart
    out.append(Case("nb-and-nb+1", np.stack(blocks, axis=1).astype(np.float32)[None], None, LATTICE))
    # pairs of single-row cells exactly r = 4 cells apart (not neighbours: strict), 3 cells apart (neighbours) and one
    # ulp inside r; nb = 1
    pairs = []
    for k, gap in enumerate((4, 3, 4, 4)):
        a = _centre((16, 16 + 10 * k, 40))
        b = a.copy()
        b[k % 3 if k < 3 else 0] += gap * V
        pairs += [a, b]
    pairs = np.stack(pairs, axis=1).astype(np.float32)
    pairs[0, 7] = np.nextafter(pairs[0, 7], np.float32(-np.inf))              # the last pair: one ulp inside
    out.append(Case("distance-r", pairs[None], None, LATTICE._replace(nb_points=1)))
    # radius 2^-13: the box is some 7 000 cells of the radius grid wide, past the exactness range of csrc/grid.h
    # (GR_COORD_LIMIT - 1 cells from the scene's first mean), so view 0 -- rows through the whole box -- is counted by
    # the index-order scan, and view 1 -- the same pattern inside a tenth of the box -- by the grid, in one call.  Rows
    # come in pairs 2^-14 apart across a cell face (two means, neighbours) or alone; nb = 1 keeps the pairs
    cols = [[], []]
    for view, span in enumerate((0.8, 0.08)):
        for k in range(40):
            cell = np.floor((0.1 + span * rng.random(3)) / V)
            a = (cell - 0.5) * V + np.array([0.0, 0.25 * V, 0.25 * V])           # on the lower x face of its cell
            if k % 2:
                cols[view] += [a + [2.0 ** -15, 0, 0], a - [2.0 ** -15, 0, 0]]
            else:
                cols[view] += [a + [2.0 ** -15, 0, 0]]
    out.append(Case("scan-scene", np.stack([np.stack(c, axis=1) for c in cols]).astype(np.float32), None,
                    LATTICE._replace(nb_points=1, radius=2.0 ** -13)))
    return tuple(Case(c.name, _frozen(c.clouds), None if c.count is None else _frozen(c.count), c.cfg) for c in out)


@functools.lru_cache(maxsize=None)
def chunk_case():
    """17 views of 64 rows on a grid of 513^3 cells (28 cell bits: 16 scenes per sort): clusters of three rows in one
    cell, pairs in adjacent cells and single rows, so that every view keeps some means and drops others."""
    B, n = 17, 64
    clouds = np.empty((B, 3, n), dtype=np.float32)
    for b in range(B):
        rng = np.random.default_rng(PE.seed_of(b, 47))
        centres = 0.125 + 0.75 * rng.random((3, 24))
        cols = []
        for k in range(24):
            step = np.array([2.0 ** -9, 0.0, 0.0]) if k % 3 == 1 else np.zeros(3)   # pairs: one cell further along x
            for r in range((3, 2, 1)[k % 3]):
                cols.append(centres[:, k] + (rng.random(3) - 0.5) * 2.0 ** -10 + r * step)
        cols = (cols + [0.125 + 0.75 * rng.random(3) for _ in range(n)])[:n]
        clouds[b] = np.stack(cols, axis=1).astype(np.float32)[:, rng.permutation(n)]
    count = np.array([n - (b % 5) for b in range(B)], np.int32)
    return Case("chunk", _frozen(clouds), _frozen(count), CHUNK)


def key_plan(cfg, B, N):
    """(cell_bits, scenes per pass) as pv_plan of csrc/process_views.hip computes them."""
    _, dims = voxel_grid(cfg)
    cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    bits = 1
    while bits < 32 and (1 << bits) < cells:
        bits += 1
    cap = 1 if bits >= 32 else (1 << (32 - bits)) - (1 if (1 << bits) == cells else 0)
    return bits, max(1, min(B, 256, (2 ** 31 - 1) // max(N, 1), cap))
