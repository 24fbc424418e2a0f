"""GPU tests of the baselines' evaluation data (`postprocess.grade_eval_view_frames`, `grade_eval_scene_frames`,
`label_eval_view`; csrc/eval_data.hip) against the fixture the reference's own `finger_hand_view` and
`finger_hand_scene` produced (tests/golden/eval_data.npz), against the float64 yardstick (tests/eval_data_ref.py) and,
bit for bit, against the shipped kernels whose sweep bodies the two entry points compile again:
`grade_precomputed_baseline_frames` with an all-true mask and a constant score of 1, and `s4g_eval_frames_f32` on the
same matrices.

The edge tests call the C ABI with every output and the workspace inside a poisoned buffer with guard bytes on both
sides, checked after the call.  Indices, flags, stages and booleans are compared exactly on the rows the yardstick calls
decided, the counts where no point lies within 4e-6 of a face; `global_to_local` within 1e-5 (an fp32 product of a
rotation and a roll, coordinates below 2: a few 2^-23); sets by `close_region_ref`'s rule (certain members in, ambiguous
optional, nothing else); maps against `projection64` of the call's own sets within `close_region_ref.map_bound`; the
antipodal score within the 1e-4 of `eval_frames` (its scale is 1; measured: 8.4e-8 from float64 on the fixture)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import close_region_ref as CRR
from tests import eval_data_ref as ED

pytestmark = pytest.mark.gpu

GUARD = 256                # bytes on both sides of every output
POISON = 0xA5
C = ED.constants_in_source()
VP = C["EVD_GX"] * C["EVD_SLOTS"]                      # frames of a view per pass
SP = C["EVS_GX"] * C["EVS_SLOTS"]                      # poses of a scene per pass
SWEEP = 256 * C["EVD_U"]
assert SWEEP == 256 * C["EVS_U"]
VCHUNK = C["EVD_CHUNK_POINTS"] * C["EVD_MIN_CHUNKS"]    # the chunk count turns one past this
SCHUNK = C["EVS_CHUNK_POINTS"] * C["EVS_MIN_CHUNKS"]


def _t(a, dev):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cfg(**kw):
    from s4g_release_amd.postprocess import EvalDataConfig, LocalSearchConfig
    return EvalDataConfig(search=LocalSearchConfig(**kw))


def _small_cfg():
    """2 depths x 3 rolls: the loop-edge shapes with hundreds of frames stay quick on the yardstick's side."""
    return _cfg(length_search=(-0.06, -0.02), theta_search_deg=(-30, 0, 30))


def _tables(s, dev):
    from s4g_release_amd.postprocess import _small_on_device
    tb = s.tables()
    return _small_on_device(torch.cat([tb["depth"], tb["lo"], tb["hi"], tb["cos"], tb["sin"]]), torch.float32, dev)


def _view_params(s):
    return (ctypes.c_float * 12)(s.finger_length, s.bottom_length, s.half_hand_thickness, s.half_bottom_width,
                                 s.half_bottom_space, s.back_collision_margin, s.back_collision_threshold,
                                 s.finger_collision_threshold, s.close_region_min_points,
                                 s.table_height + s.table_collision_offset, s.num_points_threshold, s.table_height)


def _scene_params(s):
    return (ctypes.c_float * 11)(s.finger_length, s.bottom_length, s.half_hand_thickness, s.half_bottom_width,
                                 s.half_bottom_space, s.back_collision_margin, s.back_collision_threshold,
                                 s.finger_collision_threshold, s.close_region_min_points, s.neighbor_depth,
                                 s.num_points_threshold)


class _Guarded:
    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def add(self, name, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device=self.dev)
        self.bufs[name] = (buf, buf[GUARD:GUARD + n].view(dtype).view(shape), n)
        return self.bufs[name][1].data_ptr()

    def read(self, untouched=False):
        torch.cuda.synchronize(self.dev)
        out = {}
        for k, (buf, view, n) in self.bufs.items():
            assert (buf[:GUARD] == POISON).all() and (buf[GUARD + n:] == POISON).all(), "guard of %s" % k
            if untouched:
                assert (buf == POISON).all(), "%s was written" % k
            out[k] = view.cpu().numpy()
        return out


def _view_guarded(dev, points, frames, cloud, cfg, frame_count=None, live=None, expect=0, short=0):
    """s4g_eval_view_search_f32 through the C ABI, every output and the workspace guarded.  Batched numpy in -> dict of
    numpy arrays with the names of `eval_data_ref.view64`.  short: bytes the workspace is declared too small by."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    s = cfg.search
    B, F = points.shape[:2]
    N = cloud.shape[2]
    L, T = s.shape
    ins = [_t(np.asarray(a, np.float32), dev) for a in (points, frames, cloud)]
    d_c = None if frame_count is None else _t(np.asarray(frame_count, np.int64), dev)
    d_l = None if live is None else _t(np.asarray(live, np.int32), dev)
    tables = _tables(s, dev)
    g = _Guarded(dev)
    p = {k: g.add(k, sh, dt) for k, sh, dt in (
        ("ints", (B, F, L, T, 4), torch.int32), ("slab_count", (B, F, L), torch.int32), ("index", (B, F), torch.int32),
        ("g2l", (B, F, 4, 4), torch.float32), ("flags", (B, F), torch.int32), ("valid_index", (B, F), torch.int32),
        ("count", (B,), torch.int64))}
    nbytes = int(_cabi.lib().s4g_eval_view_search_workspace_bytes(B, N, F, L, T))
    ws = g.add("workspace", (max(nbytes, 1),), torch.uint8)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_eval_view_search_f32(
            *[a.data_ptr() for a in ins], B, N, F, L, T, _view_params(s), tables.data_ptr(),
            None if d_c is None else d_c.data_ptr(), None if d_l is None else d_l.data_ptr(), p["ints"],
            p["slab_count"], p["index"], p["g2l"], p["flags"], p["valid_index"], p["count"], ws, nbytes - short,
            Fn._stream())
    assert rc == expect, rc
    out = g.read(untouched=expect != 0)
    for i, k in enumerate(("back", "finger", "close", "table_collision")):
        out[k] = out["ints"][..., i]
    return out


def _scene_guarded(dev, g2l, scene, normals, labels, cfg, count=None, live=None, expect=0, short=0):
    """s4g_eval_scene_grade_f32 through the C ABI, guarded -> dict with the names of `eval_data_ref.scene64`."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    B, K = g2l.shape[:2]
    M = scene.shape[2]
    ins = [_t(np.asarray(a, dt), dev) for a, dt in ((g2l, np.float32), (scene, np.float32), (normals, np.float32),
                                                    (labels, np.int32))]
    d_c = None if count is None else _t(np.asarray(count, np.int64), dev)
    d_l = None if live is None else _t(np.asarray(live, np.int32), dev)
    g = _Guarded(dev)
    p = {k: g.add(k, sh, dt) for k, sh, dt in (
        ("ints", (B, K, 8), torch.int32), ("non_collision", (B, K), torch.uint8), ("single_label", (B, K), torch.uint8),
        ("score", (B, K), torch.float32), ("floats", (B, K, 4), torch.float32))}
    nbytes = int(_cabi.lib().s4g_eval_scene_grade_workspace_bytes(B, M, K))
    ws = g.add("workspace", (max(nbytes, 1),), torch.uint8)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_eval_scene_grade_f32(
            *[a.data_ptr() for a in ins], B, M, K, _scene_params(cfg.search),
            None if d_c is None else d_c.data_ptr(), None if d_l is None else d_l.data_ptr(), p["ints"],
            p["non_collision"], p["single_label"], p["score"], p["floats"], ws, nbytes - short, Fn._stream())
    assert rc == expect, rc
    out = g.read(untouched=expect != 0)
    for i, k in enumerate(("slab", "back", "finger", "close", "multi", "n_left", "n_right", "stage")):
        out[k] = out["ints"][..., i]
    for i, k in enumerate(("left_y", "right_y", "mean_left", "mean_right")):
        out[k] = out["floats"][..., i]
    return out


def _check_view(got, b, y, what, keep=None):
    keep = y["decided"] if keep is None else keep
    r = np.nonzero(keep)[0]
    assert np.array_equal(got["index"][b][r], y["index"][r].astype(np.int32)), (what, "index")
    assert np.array_equal(got["flags"][b][r], y["flags"][r].astype(np.int32)), (what, "flags")
    assert np.array_equal(got["table_collision"][b][r] != 0, y["table_collision"][r]), (what, "table")
    clear = y["clear"][r]
    for k in ("back", "finger", "close"):
        assert np.array_equal(got[k][b][r][clear], y[k][r][clear].astype(np.int32)), (what, k)
    sure = y["amb_slab"][r] == 0
    assert np.array_equal(got["slab_count"][b][r][sure], y["slab_count"][r][sure].astype(np.int32)), (what, "slab")
    assert np.abs(got["g2l"][b][r] - y["g2l"][r]).max(initial=0.0) <= 1e-5, (what, "g2l")
    bad = got["index"][b] < 0
    assert not got["g2l"][b][bad].any(), (what, "invalid rows are zero")
    off = got["flags"][b] != 0
    assert not got["ints"][b][off].any() and not got["slab_count"][b][off].any(), (what, "rows that are not searched")
    n = int(got["count"][b])
    assert np.array_equal(got["valid_index"][b][:n], np.nonzero(got["index"][b] >= 0)[0]), (what, "valid_index")
    assert (got["valid_index"][b][n:] == -1).all(), (what, "padding")


def _check_scene(got, b, y, what, keep=None, score_log=None):
    keep = (y["decided"] & y["live"]) if keep is None else keep
    r = np.nonzero(keep)[0]
    for k in ("stage", "non_collision", "single_label", "n_left", "n_right", "multi"):
        assert np.array_equal(got[k][b][r].astype(np.int64), y[k][r]), (what, k)
    clear = y["clear"][r]
    for k in ("back", "finger", "close"):
        assert np.array_equal(got[k][b][r][clear], y[k][r][clear].astype(np.int32)), (what, k)
    sure = y["amb_slab"][r] == 0
    assert np.array_equal(got["slab"][b][r][sure], y["slab"][r][sure].astype(np.int32)), (what, "slab")
    a, w = got["score"][b][r].astype(np.float64), y["score"][r]
    assert np.array_equal(np.isnan(a), np.isnan(w)), (what, "NaN scores")
    d = float(np.nanmax(np.abs(a - w), initial=0.0)) if len(r) else 0.0
    if score_log is not None:
        print("%s: antipodal score %.3g from float64" % (what, d))
    assert d <= ED.SCORE_TOL, (what, "score", d)
    for k in ("mean_left", "mean_right"):
        assert np.nanmax(np.abs(got[k][b][r] - y[k][r]), initial=0.0) <= ED.SCORE_TOL, (what, k)
    dead = ~y["live"]
    for k in ("ints", "non_collision", "single_label", "score", "floats"):
        assert not got[k][b][dead].any(), (what, k, "rows that are not scanned")


# ---- the fixture ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_case():
    fx = ED.load_fixture()
    case = ED.case_of(fx)
    return fx, case, ED.label64(*case)


def test_fixture(dev, fixture_case):
    from s4g_release_amd import postprocess as PP
    fx, case, (v, t) = fixture_case
    cfg = case[6]
    kf, kg = fx["keep_frames"], fx["keep_grasps"]
    valid = fx["ref_valid"]
    F = len(valid)
    points, frames, cloud, normals = (_t(fx[k], dev) for k in ("points", "frames", "cloud", "normals"))
    s = PP.grade_eval_view_frames(points, frames, cloud, cfg)
    assert s.unbatched and tuple(s.index.shape) == (1, F)
    got = {"index": s.index, "flags": s.flags, "ints": s.ints, "slab_count": s.slab_count, "g2l": s.global_to_local,
           "valid_index": s.valid_index, "count": s.count}
    got = {k: a.cpu().numpy() for k, a in got.items()}
    for i, k in enumerate(("back", "finger", "close", "table_collision")):
        got[k] = got["ints"][..., i]
    _check_view(got, 0, v, "fixture", kf)
    assert np.array_equal((got["index"][0] >= 0)[kf], valid[kf])                    # the reference's own verdict
    row = np.full(F, -1)
    row[valid] = np.arange(valid.sum())
    g = np.nonzero(kf & valid)[0]
    assert np.abs(got["g2l"][0][g] - fx["ref_baseline_frame"][row[g]]).max() <= 1e-5
    # the crop of the view in the placement taken
    r = PP.close_regions(s.global_to_local, cloud[None], normals[None], cfg.search, None, s.index >= 0)
    off, cnt, idx = (a[0].cpu().numpy() for a in (r.offset, r.count, r.index))
    assert not r.flags.any()
    so = fx["set_offset"]
    for j, f in enumerate(fx["set_rows"]):
        mine = np.sort(idx[off[f]:off[f] + cnt[f]])
        reg = v["regions"][f]
        assert np.isin(reg["certain"], mine).all() and np.isin(mine, np.concatenate([reg["certain"], reg["ambiguous"]])).all(), f
        assert np.array_equal(mine, fx["set_index"][so[j]:so[j + 1]].astype(np.int64)), f      # (kept: nothing ambiguous)
    P, Nn, maps = r.points[0].cpu().numpy(), r.normals[0].cpu().numpy(), r.maps[0].cpu().numpy()
    proj = PP.ProjectionConfig()
    for j, f in enumerate(fx["stored_rows"]):
        p32, n32 = P[:, off[f]:off[f] + cnt[f]], Nn[:, off[f]:off[f] + cnt[f]]
        own, _ = CRR.projection64(p32, n32, proj, cfg.search)
        bound = CRR.map_bound(p32, n32, proj, cfg.search)
        assert (np.abs(maps[f] - own) <= bound).all(), f
        assert (np.abs(maps[f] - fx["maps"][j]) <= bound + float(fx["margin"][0]) + 1e-6).all(), f
    # the ground truth of the taken placements
    tr = PP.grade_eval_scene_frames(s.global_to_local, _t(fx["scene"], dev)[None], _t(fx["scene_normals"], dev)[None],
                                    _t(fx["scene_labels"], dev)[None], cfg, live=s.index >= 0)
    gs = {"ints": tr.ints, "non_collision": tr.non_collision, "single_label": tr.single_label,
          "score": tr.antipodal_score, "floats": tr.floats}
    gs = {k: a.cpu().numpy() for k, a in gs.items()}
    for i, k in enumerate(("slab", "back", "finger", "close", "multi", "n_left", "n_right", "stage")):
        gs[k] = gs["ints"][..., i]
    for i, k in enumerate(("left_y", "right_y", "mean_left", "mean_right")):
        gs[k] = gs["floats"][..., i]
    same = kg & (got["index"][0] == v["index"])
    assert same.sum() == kg.sum()
    y = dict(t, live=t["live"] & (got["index"][0] >= 0))
    _check_scene(gs, 0, y, "fixture", same, score_log=True)
    g = np.nonzero(kg)[0]
    assert np.array_equal(gs["non_collision"][0][g], fx["ref_non_collision"][row[g]])
    assert np.array_equal(gs["single_label"][0][g], fx["ref_single_label"][row[g]])
    a, b = gs["score"][0][g], fx["ref_score"][row[g]]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(a - b)) <= ED.SCORE_TOL
    for i, name in enumerate(ED.STAGES):
        assert (gs["stage"][0][g] == i).sum() >= 20, name


# ---- the cross-checks against the shipped kernels, bit for bit ------------------------------------------------------------
def test_view_search_equals_the_shipped_three_word_search(dev, fixture_case):
    """All-true mask, constant score 1: the shipped fold takes the first passing placement too, and it has no reach
    gate -- on the frames that pass it, the counts, the slabs, the index and the matrix are the same bits."""
    from s4g_release_amd import postprocess as PP
    fx, case, _ = fixture_case
    cfg = case[6]
    L, T = cfg.search.shape
    points, frames, cloud = (_t(fx[k], dev)[None] for k in ("points", "frames", "cloud"))
    F = points.shape[1]
    mine = PP.grade_eval_view_frames(points, frames, cloud, cfg)
    ones = torch.ones((1, F, L, T), dtype=torch.float32, device=dev)
    ship = PP.grade_precomputed_baseline_frames(points, frames, ones > 0, ones, cloud,
                                                PP.PrecomputedBaselineConfig(search=cfg.search))
    torch.cuda.synchronize(dev)
    reach = (mine.flags[0] & 8) == 0
    assert 20 <= int((~reach).sum()) < F - 100
    assert torch.equal(mine.ints[0][reach], ship.ints[0][reach])
    assert torch.equal(mine.slab_count[0][reach], ship.slab_count[0][reach])
    assert torch.equal(mine.index[0][reach], ship.best.index[0][reach])
    assert torch.equal(mine.global_to_local[0][reach].view(torch.int32), ship.best.global_to_local[0][reach].view(torch.int32))
    assert int((mine.index[0] >= 0).sum()) >= 200 and (mine.index[0][~reach] == -1).all()


def test_scene_grade_equals_eval_frames(dev, fixture_case):
    """The same matrices through s4g_eval_frames_f32 (invert_se3 = 0): back, finger, close, the multi-label flag and,
    wherever that class reaches its score too, the bands and the score are the same bits."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    from s4g_release_amd import postprocess as PP
    fx, case, _ = fixture_case
    cfg = case[6]
    s = cfg.search
    points, frames, cloud = (_t(fx[k], dev)[None] for k in ("points", "frames", "cloud"))
    scene, nrm, lab = (_t(fx[k], dev)[None] for k in ("scene", "scene_normals", "scene_labels"))
    g2l = PP.grade_eval_view_frames(points, frames, cloud, cfg).global_to_local
    live = g2l.abs().sum((2, 3)) > 0
    mine = PP.grade_eval_scene_frames(g2l, scene, nrm, lab, cfg, live=live)
    K, M = g2l.shape[1], scene.shape[2]
    ints = torch.empty((1, K, 8), dtype=torch.int32, device=dev)
    floats = torch.empty((1, K, 5), dtype=torch.float32, device=dev)
    nbytes = int(_cabi.lib().s4g_eval_frames_workspace_bytes(1, M, K))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    params = (ctypes.c_float * 10)(*list(_scene_params(s))[:10])
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_eval_frames_f32(scene.data_ptr(), nrm.data_ptr(), lab.data_ptr(), g2l.data_ptr(), 1, M, K,
                                             params, None, 0, ints.data_ptr(), floats.data_ptr(), ws.data_ptr(), nbytes,
                                             Fn._stream())
    assert rc == 0
    torch.cuda.synchronize(dev)
    lv = live[0]
    assert int(lv.sum()) >= 200
    assert not ints[0, :, 7].any()                                   # its eighth integer stays 0
    for mi, si in ((1, 0), (2, 1), (3, 2), (4, 3)):                  # back, finger, close, multi
        assert torch.equal(mine.ints[0, :, mi][lv], ints[0, :, si][lv]), (mi, si)
    both = lv & (mine.stage[0] == 0)
    scored_there = (ints[0, :, 4] + ints[0, :, 5]) > 0
    assert int(both.sum()) >= 100 and scored_there[both].all()
    assert torch.equal(mine.ints[0, :, 5:7][both], ints[0, :, 4:6][both])
    assert torch.equal(mine.floats[0][both].view(torch.int32), floats[0, :, :4][both].view(torch.int32))
    assert torch.equal(mine.antipodal_score[0][both].view(torch.int32), floats[0, :, 4][both].view(torch.int32))


# ---- loop edges -------------------------------------------------------------------------------------------------------------
_EDGES = [(1, 1, 1, 1), (2, 200, 5, 4), (1, 63, 2, 3), (1, 64, 3, 2), (1, 65, 2, 2), (1, SWEEP - 1, VP - 1, SP - 1),
          (3, SWEEP, VP, SP), (1, SWEEP + 1, VP + 1, SP + 1), (1, VCHUNK - 1, 3, 3), (3, VCHUNK, 2, 2),
          (1, VCHUNK + 1, 2, 3)]
assert VCHUNK == SCHUNK


@pytest.mark.parametrize("B,N,F,K", _EDGES)
def test_edges(dev, B, N, F, K):
    """Chunk, sweep and pass boundaries of both entry points; per-scene counts that differ and include 0; 2 x 3 and
    4 x 12 placements.  The scene stage grades the matrices the yardstick's view stage took, repeated to K rows, against
    the same cloud."""
    cfg = _small_cfg() if max(F, K) > 8 else _cfg()
    rng = np.random.default_rng(1000 * B + N + F)
    cases = [ED.lattice_case(rng, N, F, cfg) for _ in range(B)]
    counts = [F, 0, F // 2 + 1][:B] if B > 1 else [F]
    got = _view_guarded(dev, *[np.stack([c[i] for c in cases]) for i in range(3)], cfg,
                        frame_count=counts if B > 1 else None)
    ys = []
    for b, c in enumerate(cases):
        y = ED.view64(c[0], c[1], c[2], cfg, frame_count=counts[b])
        assert y["decided"].all()
        _check_view(got, b, y, (B, N, F, b))
        dead = np.arange(F) >= counts[b]
        assert (got["index"][b][dead] == -1).all() and (got["flags"][b][dead] == 1).all()
        assert int(got["count"][b]) == y["count"]
        ys.append(y)
    kc = [K, 0, K // 2 + 1][:B] if B > 1 else [K]
    g2l = np.stack([y["g2l"].astype(np.float32)[np.arange(K) % F] for y in ys])
    if F > 1:
        g2l[:, K // 2] = 0                                           # a row that `live` switches off
    live = np.abs(g2l).sum((2, 3)) > 0
    gs = _scene_guarded(dev, g2l, *[np.stack([c[i] for c in cases]) for i in (2, 3, 4)], cfg,
                        count=kc if B > 1 else None, live=live)
    for b, c in enumerate(cases):
        gb = g2l[b].copy()
        gb[kc[b]:] = 0
        y = ED.scene64(gb, c[2], c[3], c[4], cfg)
        assert (y["decided"] | ~y["live"]).mean() >= 0.9
        _check_scene(gs, b, y, (B, N, K, b))


def test_short_workspace_and_dead_rows(dev):
    cfg = _cfg()
    P, Fr, cloud, nrm, lab = ED.lattice_case(np.random.default_rng(3), 200, 3, cfg)
    _view_guarded(dev, P[None], Fr[None], cloud[None], cfg, expect=-2, short=1)        # S4G_EWORKSPACE, nothing written
    y = ED.view64(P, Fr, cloud, cfg)
    g2l = y["g2l"].astype(np.float32)[None]
    _scene_guarded(dev, g2l, cloud[None], nrm[None], lab[None], cfg, expect=-2, short=1)
    got = _view_guarded(dev, P[None], Fr[None], cloud[None], cfg, live=np.zeros((1, 3), np.int32))
    assert (got["index"] == -1).all() and (got["flags"] == 1).all() and int(got["count"][0]) == 0
    assert not got["ints"].any() and not got["g2l"].any() and not got["slab_count"].any()
    gs = _scene_guarded(dev, g2l, cloud[None], nrm[None], lab[None], cfg, live=np.zeros((1, 3), np.int32))
    assert not gs["ints"].any() and not gs["non_collision"].any() and not gs["score"].any()
    empty = _view_guarded(dev, P[None, :0], Fr[None, :0], cloud[None], cfg)           # F = 0: the count, by a kernel
    assert int(empty["count"][0]) == 0


# ---- properties ---------------------------------------------------------------------------------------------------------
def _bits(x):
    out = []
    for a in x:
        out.append(a.view(torch.int32) if a.dtype == torch.float32 else a)
    return out


def _view_bits(s):
    return _bits([s.ints, s.slab_count, s.index, s.global_to_local, s.flags, s.valid_index, s.count])


def _scene_bits(t):
    return _bits([t.ints, t.non_collision, t.single_label, t.antipodal_score, t.floats])


@pytest.fixture(scope="module")
def blob_case():
    cfg = _cfg()
    rng = np.random.default_rng(77)
    return (cfg,) + tuple(np.stack(a) for a in zip(*[ED.lattice_case(rng, 700, 9, cfg) for _ in range(3)]))


def test_repeatable_and_batch_invariant(dev, blob_case):
    from s4g_release_amd import postprocess as PP
    cfg, P, Fr, cloud, nrm, lab = blob_case
    d = [_t(a, dev) for a in (P, Fr, cloud, nrm, lab)]
    run = lambda sl: PP.grade_eval_view_frames(d[0][sl], d[1][sl], d[2][sl], cfg)             # noqa: E731
    one, again = run(slice(None)), run(slice(None))
    assert int(one.count.sum()) >= 6
    assert all(torch.equal(a, b) for a, b in zip(_view_bits(one), _view_bits(again)))
    grade = lambda g, sl: PP.grade_eval_scene_frames(g, d[2][sl], d[3][sl], d[4][sl], cfg, live=g.abs().sum((2, 3)) > 0)   # noqa: E731
    t1, t2 = grade(one.global_to_local, slice(None)), grade(one.global_to_local, slice(None))
    assert all(torch.equal(a, b) for a, b in zip(_scene_bits(t1), _scene_bits(t2)))
    for b in range(3):
        alone = run(slice(b, b + 1))
        assert all(torch.equal(a[0], w[b]) for a, w in zip(_view_bits(alone), _view_bits(one)))
        ta = grade(alone.global_to_local, slice(b, b + 1))
        assert all(torch.equal(a[0], w[b]) for a, w in zip(_scene_bits(ta), _scene_bits(t1)))


def test_graph_capture(dev, blob_case):
    from s4g_release_amd import postprocess as PP
    cfg, P, Fr, cloud, nrm, lab = blob_case
    d = [_t(a, dev) for a in (P, Fr, cloud, nrm, lab)]

    def run():
        s = PP.grade_eval_view_frames(d[0], d[1], d[2], cfg)
        return s, PP.grade_eval_scene_frames(s.global_to_local, d[2], d[3], d[4], cfg, live=s.index >= 0)
    s0, t0 = run()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # a host read or a memset node would fail here
        s1, t1 = run()
    for a in _view_bits(s1) + _scene_bits(t1):
        a.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert all(torch.equal(a, b) for a, b in zip(_view_bits(s0) + _scene_bits(t0), _view_bits(s1) + _scene_bits(t1)))


def test_nan_invalidates_its_own_row_only(dev, blob_case):
    from s4g_release_amd import postprocess as PP
    cfg, P, Fr, cloud, nrm, lab = blob_case
    d = [_t(a[:1], dev) for a in (P, Fr, cloud, nrm, lab)]
    base = PP.grade_eval_view_frames(d[0], d[1], d[2], cfg)
    bad_p, bad_f = d[0].clone(), d[1].clone()
    bad_p[0, 2, 1] = float("nan")
    bad_f[0, 5, 1, 2] = float("inf")
    got = PP.grade_eval_view_frames(bad_p, bad_f, d[2], cfg)
    rows = torch.ones(9, dtype=torch.bool, device=dev)
    rows[[2, 5]] = False
    assert all(torch.equal(a[0][rows], b[0][rows]) for a, b in zip(_view_bits(base)[:5], _view_bits(got)[:5]))
    assert (got.index[0][~rows] == -1).all() and (got.flags[0][~rows] == 2).all()
    assert not got.global_to_local[0][~rows].any() and not got.ints[0][~rows].any()
    live = base.index >= 0
    t0 = PP.grade_eval_scene_frames(base.global_to_local, d[2], d[3], d[4], cfg, live=live)
    g = base.global_to_local.clone()
    k = int(torch.nonzero(live[0])[0])
    g[0, k, 1, 3] = float("nan")
    t1 = PP.grade_eval_scene_frames(g, d[2], d[3], d[4], cfg, live=live)
    rows = torch.ones(9, dtype=torch.bool, device=dev)
    rows[k] = False
    assert all(torch.equal(a[0][rows], b[0][rows]) for a, b in zip(_scene_bits(t0), _scene_bits(t1)))
    assert bool(t1.not_finite[0, k]) and int(t1.non_collision[0, k]) == 0 and int(t1.single_label[0, k]) == 0
    assert float(t1.antipodal_score[0, k]) == 0.0 and not t1.not_finite[0][rows].any()
    cl = d[2].clone()                                                 # a cloud point that is not finite is in no region
    cl[0, :, -1] = float("nan")
    pad = torch.cat([d[2], torch.full((1, 3, 1), float("nan"), device=dev)], 2)
    a, b = PP.grade_eval_view_frames(d[0], d[1], pad, cfg), base
    assert all(torch.equal(x, y) for x, y in zip(_view_bits(a), _view_bits(b)))


# ---- the chain ----------------------------------------------------------------------------------------------------------
def test_chain_from_views_to_classifier_scores(dev, fixture_case):
    """process_views -> label_eval_view -> score_projections / score_close_regions with seeded classifiers: the scores
    equal scoring the same maps and sets passed densely; `dump` holds the reference's dictionary."""
    from s4g_release_amd import postprocess as PP
    from s4g_release_amd import preprocess as PRE
    from s4g_release_amd.baselines import FusedGPD, FusedPointNetGPD, GPDClassifier, PointNetGPDClassifier
    from tests import gpd_ref as GR
    from tests import pointnet_gpd_ref as PR
    fx = fixture_case[0]
    scene, nrm, lab = (_t(fx[k], dev)[None] for k in ("scene", "scene_normals", "scene_labels"))
    pv = PRE.process_views(scene)
    n = int(pv.count[0])
    assert n >= 1000
    cloud = pv.points[:, :, :n].contiguous()
    # (candidates from 5 cm above the table on: in ascending index the first ones of a voxel-ordered cloud are the lowest)
    cfg = PP.EvalDataConfig(grasp_num=256, sample_region=0.80)
    camera = torch.tensor([[0.8, 0.0, 1.7]], device=dev)
    v = PP.label_eval_view(cloud, None, scene, nrm, lab, cfg, camera=camera)
    again = PP.label_eval_view(cloud, None, scene, nrm, lab, cfg, camera=camera)
    assert all(torch.equal(a, b) for a, b in zip(_view_bits(v.search) + _scene_bits(v.truth),
                                                 _view_bits(again.search) + _scene_bits(again.truth)))
    count = int(v.search.count[0])
    print("chain: %d of %d frames taken" % (count, int(v.frames.frame_count[0])))
    assert tuple(v.search.index.shape) == (1, 256) and 5 <= count <= 256
    few = v.frames.count[0] < cfg.min_neighbours
    assert (v.search.index[0][few] == -1).all()                       # decision 3: not a candidate
    taken = v.search.index[0] >= 0
    assert not v.truth.ints[0][~taken].any() and (v.regions.count[0][~taken] == 0).all()
    vi = v.search.valid_index[0, :count].long()
    # GPD on the maps, PointNetGPD on the sets: in place through valid_index, and densely
    gs = GR.hashed_state(12, 2)
    gnet = GPDClassifier(12, 2)
    gnet.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for k, a in gs.items()})
    gpd = FusedGPD(gnet.to(dev).eval())
    ps = PR.hashed_state(2)
    pnet = PointNetGPDClassifier(3, 2)
    pnet.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in ps.items()})
    pgpd = FusedPointNetGPD(pnet.to(dev).eval())
    got = PP.score_projections(v, gpd, grasp_num=count)
    dense = gpd(v.regions.maps[0][vi].contiguous())
    assert torch.equal(got[0].view(torch.int32), dense.view(torch.int32))
    assert torch.equal(PP.score_projections(v.regions, gpd)[0][vi].view(torch.int32), dense.view(torch.int32))
    got = PP.score_close_regions(v, pgpd, grasp_num=count)
    off, cnt = v.regions.offset[0].cpu().numpy(), v.regions.count[0].cpu().numpy()
    assert not v.regions.flags[0][vi].any() and cnt[vi.cpu().numpy()].min() >= cfg.search.close_region_min_points
    alone = torch.cat([pgpd(v.regions.points[:, :, off[f]:off[f] + cnt[f]].contiguous()) for f in vi.cpu().numpy()])
    assert torch.equal(got[0].view(torch.int32), alone.view(torch.int32))
    d = v.dump(0)
    assert list(d) == ["frame", "antipodal_score", "non_collision_bool", "single_label_bool", "view_cloud", "scene_cloud",
                       "scene_label", "scene_normal", "close_region_points_set", "close_region_normals_set",
                       "close_region_projection_map_set"]
    assert d["frame"].shape == (count, 4, 4) and len(d["close_region_points_set"]) == count
    G = v.search.global_to_local[0][vi].cpu().numpy().astype(np.float64)
    assert np.abs(d["frame"] @ G - np.eye(4)).max() <= 1e-5
    assert d["non_collision_bool"].dtype == np.uint8 and d["view_cloud"].shape == (n, 3)
    # a seeded shuffle takes other candidates in another order, on the device
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    sh = PP.label_eval_view(cloud, v.normals, scene, nrm, lab, cfg, generator=gen)
    assert not torch.equal(sh.frames.frame_index, v.frames.frame_index)
    assert (sh.frames.frame_index[0, :int(sh.frames.frame_count[0])] >= 0).all()
