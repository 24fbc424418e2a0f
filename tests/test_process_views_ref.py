"""CPU side of `process_views` (tests/process_views_ref.py): the yardstick's stages against oracle/preprocess.py where
both apply, eight sabotaged restatements against the constructions (a yardstick that cannot tell them apart pins
nothing), the constants against the sources, every construction against what it is there for, and the host-side
refusals of the wrapper (no device needed)."""
import os
import re

import numpy as np
import pytest

from oracle import preprocess as OP
from tests import preprocess_edges as PE
from tests import process_views_ref as PV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "s4g_release_amd", "csrc")


def _one(pattern, text, what):
    found = re.findall(pattern, text, flags=re.M)
    assert len(found) == 1, "%s: expected exactly one match of %r, found %d" % (what, pattern, len(found))
    return found[0]


def _all_cases():
    return list(PV.constructions()) + [PV.size_case(n) for n in (65, 257)] + [PV.chunk_case()]


# --------------------------------------------------------------------------------------------------------- constants
def test_the_constants_are_the_sources():
    from s4g_release_amd import preprocess as PP
    cfg = PP.ViewProcessingConfig()
    assert (cfg.workspace, cfg.voxel_size, cfg.voxel_bounds, cfg.nb_points, cfg.radius) == tuple(PV.DATA_GEN)
    src = open(os.path.join(CSRC, "process_views.hip")).read()
    assert int(_one(r"^constexpr int PV_THREADS = (\d+);", src, "PV_THREADS")) == PE.PP_THREADS
    assert int(_one(r"^constexpr int PV_BLOCK = (\d+);", src, "PV_BLOCK")) == PE.VOXEL_THREADS
    assert int(_one(r"^constexpr int PV_CHUNK = (\d+);", src, "PV_CHUNK")) == 256
    assert int(_one(r"^constexpr int PV_DIM = (\d+);", src, "PV_DIM")) == 64
    _one(r"const float h = radius \* \(1\.0f \+ 1\.0f / 256\.0f\);", src, "cell edge")
    _one(r"const float r2 = radius \* radius;", src, "r2")
    assert len(re.findall(r"dist2<FMAD>\([^)]*\) < r2 \? 1 : 0;", src)) == 3
    _one(r"ws\.keep\[\(size_t\)b \* N \+ v\] = cnt > nb \? 1 : 0;", src, "threshold")
    _one(r"keep = x > lox && y > loy && z > loz && x < hix && y < hiy && z < hiz;", src, "crop predicate")
    assert len(re.findall(r"floorf\(__fdiv_rn\(__fsub_rn\(p0\[[^\]]*\], o[xyz]\), voxel\)\)", src)) == 3


def test_the_grid_is_the_wrappers():
    from s4g_release_amd import preprocess as PP
    for cfg in (PV.DATA_GEN, PV.LATTICE, PV.CHUNK):
        origin, dims = PP.ViewProcessingConfig(*cfg).grid()
        o2, d2 = PV.voxel_grid(cfg)
        assert origin.tobytes() == o2.tobytes() and np.array_equal(dims, d2)
    assert tuple(PV.voxel_grid(PV.DATA_GEN)[1]) == (201, 201, 161)
    assert tuple(PV.voxel_grid(PV.CHUNK)[1]) == (513, 513, 513)
    assert PV.key_plan(PV.CHUNK, 17, 64) == (28, 16)            # the chunk case crosses a pass
    assert PV.key_plan(PV.DATA_GEN, 16, 48902) == (23, 16)


def test_the_wrapper_refuses_bad_configurations_on_the_host():
    from s4g_release_amd import preprocess as PP
    good = PP.ViewProcessingConfig()
    good.grid()
    with pytest.raises(ValueError, match="do not contain the workspace"):
        PP.ViewProcessingConfig(voxel_bounds=((-0.3, -0.5, 0.7), (0.5, 0.5, 1.5))).grid()
    with pytest.raises(ValueError, match="do not contain the workspace"):
        PP.ViewProcessingConfig(voxel_bounds=((-0.5, -0.5, 0.7), (0.5, 0.5, 1.1))).grid()
    with pytest.raises(ValueError):
        PP.ViewProcessingConfig(voxel_size=0.0).grid()
    with pytest.raises(ValueError):
        PP.ViewProcessingConfig(voxel_bounds=((-0.5, -0.5, float("nan")), (0.5, 0.5, 1.5))).grid()
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        import torch
        PP.process_views(torch.zeros(1, 3, 8))


# ------------------------------------------------------------------------------------------- stages against the oracle
@pytest.mark.parametrize("case", [c.name for c in PV.constructions()] + ["n257", "chunk"])
def test_stages_equal_the_oracle(case):
    c = {k.name: k for k in _all_cases()}[case]
    origin, dims = PV.voxel_grid(c.cfg)
    for b in range(c.clouds.shape[0]):
        live = c.clouds.shape[2] if c.count is None else int(c.count[b])
        p = c.clouds[b]
        kept = PV.crop_ref(p, live, c.cfg.workspace)
        assert np.array_equal(kept, OP.filter_work_space(p[:, :live], c.cfg.workspace))
        q = p[:, kept]
        means, trace = PV.voxel_trace_ref(q, c.cfg.voxel_size, origin, dims)
        assert means.tobytes() == PE.voxel_ref(q, c.cfg.voxel_size, origin, dims).tobytes()
        if q.shape[1]:
            # the oracle's own grid starts at the cloud's minimum: the same cells where the bounds' minimum is that
            o2, d2 = OP.voxel_grid(q, c.cfg.voxel_size)
            m2, t2 = PV.voxel_trace_ref(q, c.cfg.voxel_size, o2, d2)
            assert m2.tobytes() == OP.voxel_down_sample(q, c.cfg.voxel_size).tobytes()
            assert (np.diff(np.sort(t2)) > 0).all() and len(t2) == m2.shape[1]
        cnt = PV.neighbour_counts(means, c.cfg.radius)
        assert np.array_equal(cnt, OP.radius_neighbour_counts(means, c.cfg.radius))
        assert np.array_equal(cnt, PE.counts_ref(means, c.cfg.radius))
        assert np.array_equal(cnt > c.cfg.nb_points, OP.remove_radius_outlier(means, c.cfg.nb_points, c.cfg.radius))


def test_the_trace_is_the_highest_index_of_the_cell():
    c = PV.size_case(257)
    origin, dims = PV.voxel_grid(c.cfg)
    p = c.clouds[0][:, PV.crop_ref(c.clouds[0], 257, c.cfg.workspace)]
    means, trace = PV.voxel_trace_ref(p, c.cfg.voxel_size, origin, dims)
    idx = np.floor(((p - origin[:, None]).astype(np.float32) / np.float32(c.cfg.voxel_size))).astype(np.int64)
    key = (idx[2] * dims[1] + idx[1]) * dims[0] + idx[0]
    assert (idx >= 0).all() and (idx < dims[:, None]).all()                  # the grid contains the box: no clamp
    cells = np.unique(key)
    assert len(cells) == len(trace) < p.shape[1]
    for k, t in zip(cells, trace):
        assert t == np.nonzero(key == k)[0].max()


# ------------------------------------------------------------------------------------------------------- sabotages
@pytest.fixture(scope="module")
def honest():
    return {c.name: PV.process_views_ref(c.clouds, c.count, c.cfg) for c in _all_cases()}


SEEN_BY = {
    "crop-non-strict": "box-faces", "trace-lowest": "one-cell", "trace-not-composed": "non-finite",
    "self-not-counted": "nb-and-nb+1", "count-ge": "nb-and-nb+1", "distance-le": "distance-r",
    "mean-fp32": "one-cell", "scene-base-dropped": "empty-scenes",
}


def test_there_are_eight_sabotages():
    assert len(PV.SABOTAGES) >= 8 and set(SEEN_BY) == set(PV.SABOTAGES)


@pytest.mark.parametrize("sabotage", PV.SABOTAGES)
def test_a_sabotaged_restatement_is_seen(honest, sabotage):
    c = {k.name: k for k in _all_cases()}[SEEN_BY[sabotage]]
    wrong = PV.process_views_ref(c.clouds, c.count, c.cfg, sabotage=sabotage)
    assert not PV.same(wrong, honest[c.name]), "%s goes unseen on %s" % (sabotage, c.name)


# --------------------------------------------------------------------------------------------------- constructions
def test_constructions_are_what_they_say(honest):
    by = {c.name: c for c in PV.constructions()}
    r = honest["empty-scenes"]
    assert r.crop_count[0] > 0 and r.count[0] > 0 and 0 < r.count[0] < r.voxel_count[0] < r.crop_count[0]
    assert (r.crop_count[1:] == 0).all() and (r.voxel_count[1:] == 0).all() and (r.count[1:] == 0).all()
    assert np.isnan(r.points[1:]).all() and (r.index_in_ref[1:] == -1).all()
    r, n = honest["one-cell"], by["one-cell"].clouds.shape[2]
    assert (r.crop_count[0], r.voxel_count[0], r.count[0], r.index_in_ref[0, 0]) == (n, 1, 1, n - 1)
    r, n = honest["own-cell"], by["own-cell"].clouds.shape[2]
    assert r.crop_count[0] == r.voxel_count[0] == r.count[0] == n
    assert sorted(r.index_in_ref[0]) == list(range(n)) and list(r.index_in_ref[0]) != list(range(n))    # reordered
    assert r.points[0].tobytes() == by["own-cell"].clouds[0][:, r.index_in_ref[0]].tobytes()            # mean of one
    r = honest["duplicates"]
    assert r.voxel_count[0] * 5 <= r.crop_count[0] and (r.index_in_ref[0, :r.count[0]] >= 240).all()
    r, c = honest["non-finite"], by["non-finite"]
    assert (~np.isfinite(c.clouds[0][:, :250])).any(axis=0).sum() >= 9 and r.crop_count[0] < 241
    assert np.isfinite(r.points[0, :, :r.count[0]]).all() and r.index_in_ref[0, :r.count[0]].max() < 250
    r = honest["box-faces"]
    assert r.crop_count[0] == 6 and sorted(r.index_in_ref[0, :6] % 3) == [1] * 6   # the six rows one ulp inside
    r, c = honest["cell-faces"], by["cell-faces"]
    # a row ON face k belongs to cell k, with the row one ulp above; the row one ulp below is in cell k - 1: per axis
    # the faces 20, 21, 22 and 64 make the cells 19 .. 22, 63 and 64
    assert r.crop_count[0] == 36 and r.voxel_count[0] == 18
    origin, _ = PV.voxel_grid(c.cfg)
    on = c.clouds[0][:, 1::3]
    cell = np.floor(((on - origin[:, None]).astype(np.float32) / np.float32(c.cfg.voxel_size)))
    assert [int(cell[a, 4 * a + i]) for a in range(3) for i in range(4)] == [20, 21, 22, 64] * 3
    r = honest["nb-and-nb+1"]
    nb = PV.LATTICE.nb_points
    assert r.voxel_count[0] == 4 * nb + 2 and r.count[0] == (nb + 1) + (nb + 2)
    assert sorted(r.index_in_ref[0, :r.count[0]]) == list(range(nb, 2 * nb + 1)) + list(range(3 * nb, 4 * nb + 2))
    r = honest["distance-r"]
    assert r.voxel_count[0] == 8 and sorted(r.index_in_ref[0, :r.count[0]]) == [2, 3, 6, 7]
    r, c = honest["scan-scene"], by["scan-scene"]
    assert (r.crop_count == 60).all() and (r.voxel_count[0], r.count[0]) == (60, 40)    # 20 pairs kept, 20 rows not
    assert 30 < r.count[1] < r.voxel_count[1] <= 60                                     # (cells may coincide there)
    for b, outside in ((0, True), (1, False)):       # the first mean is the grid's origin; the means are all kept or not
        means = PV.voxel_trace_ref(c.clouds[b], c.cfg.voxel_size, *PV.voxel_grid(c.cfg))[0]
        cells = np.stack([PE.cell_coord(means[a], means[a, 0], c.cfg.radius) for a in range(3)])
        assert (np.abs(cells).max() >= PE.GR_COORD_LIMIT - 1) == outside, b
    r = honest["chunk"]
    assert ((r.count > 0) & (r.count < r.voxel_count) & (r.voxel_count < r.crop_count)).all()
    for n in (65, 257):
        r = honest["n%d" % n]
        assert 0 < r.count[0] < r.voxel_count[0] < r.crop_count[0] < n and r.crop_count[2] == 0
        assert r.index_in_ref[1, :r.count[1]].max() < n // 2 + 1


def test_padding_and_order(honest):
    for name, r in honest.items():
        for b in range(len(r.count)):
            k = r.count[b]
            assert np.isfinite(r.points[b, :, :k]).all() and np.isnan(r.points[b, :, k:]).all(), name
            assert (r.index_in_ref[b, :k] >= 0).all() and (r.index_in_ref[b, k:] == -1).all(), name
            assert len(set(r.index_in_ref[b, :k].tolist())) == k, name
