"""Float64 yardstick of the baselines' evaluation data (`postprocess.grade_eval_view_frames`,
`grade_eval_scene_frames`, `label_eval_view`, csrc/eval_data.hip; the reference's `EvalDataGenerator.finger_hand_view`,
`finger_hand_scene`, `_table_collision_check` and `_antipodal_score`, data_gen/eval/evaluation_data_generator.py:161-186,
209-391).  TEST INFRASTRUCTURE ONLY.

It composes what exists: `precomputed_view_ref.grade64` for the per-placement counts of the VIEW stage (all-true mask,
no label gate, with the reach gate), `close_region_ref.g2l64` / `regions64` for the matrix and the crop, and its own
`scene64` for the scene stage, which has this class's slab counter and order of returns.

  * `view64`    per frame: `back`, `finger`, `close`, `table_collision` (F, L, T), `slab_count`, `amb_slab` (F, L),
                `passed` (F, L, T), `index` (the FIRST passing placement, depths outer, rolls inner, or -1), `g2l`
                (float64), `flags`, `decided`, `clear` (F, L, T: no point within `tol` of a face of the placement).
  * `scene64`   per pose: `slab`, `back`, `finger`, `close`, `multi`, `n_left`, `n_right`, `stage`, `non_collision`,
                `single_label`, `score`, `left_y`, `right_y`, `mean_left`, `mean_right`, `amb_slab`, `decided`, `clear`
                (no point within `tol` of a face of the box: the counts hold for any fp32 route).
  * `label64`   both, with the crop `regions` of the view between them.
  * `SABOTAGES` the mistakes the fixture must see; `altered_rows` counts the kept rows one of them changes.

The kernels' loop structure (what the edge shapes of tests/test_eval_data_gpu.py cross) is read from
csrc/eval_data.hip by `constants_in_source`."""
import dataclasses
import os
import re
from types import SimpleNamespace

import numpy as np

from tests import close_region_ref as CRR
from tests import local_search_ref as LR
from tests import precomputed_view_ref as PV

ROOT = PV.ROOT
TOL = 4e-6
SCORE_TOL = 1e-4        # the bound `eval_frames` is held to: scores and means within 1e-4 of float64 (their scale is 1)
STAGES = ("scored", "slab", "back", "finger", "labels", "few")
VIEW_SABOTAGES = ("last_placement", "no_reach_gate", "no_slab_skip", "finger_ge", "no_y_offset", "no_z_offset")
SCENE_SABOTAGES = ("labels_before_collision", "empty_label_0", "slab_at_dl", "bands_swapped", "few_before_labels")
# `<=` at the scene's min-points line (:388) is a mistake `scene64` can make ("min_points_le"), but no fixture row sees
# it: it needs a grasp that passes every other gate with exactly CLOSE_REGION_MIN_POINTS scene points between the fingers.
SABOTAGES = VIEW_SABOTAGES + SCENE_SABOTAGES
# A mistake that the reference's constants hide is looked for with another constant.  The slab skip (:258) cannot show
# while CLOSE_REGION_MIN_POINTS (10) exceeds NUM_POINTS_THRESHOLD (8): a placement whose slab is skipped could not pass
# anyway.  It is looked for with no minimum, where an empty placement in a sparse slab must still not be taken.
SABOTAGE_CONFIG = {"no_slab_skip": {"close_region_min_points": 0}}
REQUIRED = {"scored": 20, "slab": 20, "back": 20, "finger": 20, "labels": 20, "few": 20, "not_first": 20,
            "frame_gate": 20, "reach_gate": 20, "depth_skipped": 20}


def constants_in_source():
    """The launch constants of csrc/eval_data.hip as a dict of ints (EVD_* the view search, EVS_* the scene grade)."""
    text = open(os.path.join(ROOT, "s4g_release_amd", "csrc", "eval_data.hip")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (EV[DS]_[A-Z_]+) = (\d+);", text)}


def default_config(**kw):
    from s4g_release_amd.postprocess import EvalDataConfig
    return EvalDataConfig(**kw)


def view64(points, frames, cloud, cfg, tol=TOL, frame_count=None, live=None, sabotage=()):
    """points (F, 3), frames (F, 3, 3), cloud (3, N) fp32 -> dict of numpy arrays (see the module docstring)."""
    s = cfg.search
    k = LR.constants(s)
    L, T = s.shape
    F = len(points)
    frames = np.asarray(frames, np.float32).copy()
    lv = np.ones(F, bool) if live is None else np.asarray(live) != 0
    if frame_count is not None:
        lv &= np.arange(F) < int(frame_count)
    vc = SimpleNamespace(search=s, valid_search_min=0.0, valid_antipodal_min=0.0)
    sab = ("no_label_gate",) + (() if "no_reach_gate" in sabotage else ("reach_gate",))
    fr = np.where(lv[:, None, None], frames, 0)         # (a row that is not scanned: the zero frame, which is skipped)
    y = PV.grade64(points, fr, np.ones((F, L, T), bool), np.zeros((F, L, T), np.int64),
                   np.zeros((F, L, T), np.float32), cloud, np.zeros(np.asarray(cloud).shape[1], np.int64), vc, tol,
                   None, sab)
    out = {n: y[n] for n in ("back", "finger", "close", "table_collision", "slab_count", "amb_slab", "decided")}
    fin = np.isfinite(frames).all((1, 2)) & np.isfinite(np.asarray(points, np.float32)).all(1)
    gate = y["gate"] & lv & fin
    out["decided"] = np.where(lv & fin, y["decided"], True)
    out["table_collision"] = y["table_collision"] & gate[:, None, None]
    slab_ok = np.ones((F, L), bool) if "no_slab_skip" in sabotage else ~(y["slab_count"] < k["slab_thr"])
    fing_bad = y["finger"] >= k["fing_thr"] if "finger_ge" in sabotage else y["finger"] > k["fing_thr"]
    passed = gate[:, None, None] & ~y["table_collision"] & slab_ok[:, :, None] & ~(y["back"] > k["back_thr"]) & \
        ~fing_bad & ~(y["close"] < k["min_points"])
    out["passed"] = passed
    flat = passed.reshape(F, -1)
    index = np.full(F, -1, np.int64)
    for f in range(F):
        nz = np.nonzero(flat[f])[0]
        if len(nz):
            index[f] = nz[-1] if "last_placement" in sabotage else nz[0]
    out["index"] = index
    out["g2l"] = CRR.g2l64(np.asarray(points, np.float32), frames, s, index)
    mean = np.abs(frames.astype(np.float64)).mean((1, 2))
    # The reference returns at the first passing placement: what comes after it cannot turn the row.  A row is decided
    # when `precomputed_view_ref.grade64` says so (every verdict of all L * T placements holds) or when every placement
    # up to the taken one has a certain table verdict and, where it is graded, a certain slab verdict and clear counts.
    R64 = frames.astype(np.float64)
    corners = np.array([[cx, cy, cz] for cx in (k["fl"], -k["bl"]) for cy in (k["hbw"], -k["hbw"])
                        for cz in (k["hht"], -k["hht"])])
    slab_sure = (y["slab_count"] - y["amb_slab"] >= k["slab_thr"]) | (y["slab_count"] + y["amb_slab"] < k["slab_thr"])
    for f in np.nonzero(~out["decided"] & gate)[0]:
        ok = abs(np.abs(R64[f]).mean() - 1e-6) > 1e-8
        last = index[f] if index[f] >= 0 and "last_placement" not in sabotage else L * T - 1
        for pl in range(last + 1):
            d, t = divmod(pl, T)
            c, sn = k["cos"][t], k["sin"][t]
            m = np.array([R64[f, 2, 0], R64[f, 2, 1] * c + R64[f, 2, 2] * sn, -R64[f, 2, 1] * sn + R64[f, 2, 2] * c])
            zc = corners @ m + (R64[f, 2, 0] * k["depth"][d] + float(np.float32(points[f][2])))
            ok &= not (np.abs(zc - k["tl"]) < tol).any()
            if not y["table_collision"][f, d, t]:
                ok &= bool(slab_sure[f, d]) and (bool(y["slab_count"][f, d] < k["slab_thr"]) or bool(y["clear"][f, d, t]))
        out["decided"][f] = ok
    out["flags"] = np.where(~lv, 1, np.where(~fin, 2, np.where(mean < 1e-6, 4, np.where(~gate, 8, 0))))
    out["clear"] = y["clear"] | ~gate[:, None, None]      # (F, L, T): the placement's three counts hold for any fp32 route
    out["depth_skipped"] = gate & (y["slab_count"] < k["slab_thr"]).any(1)
    vi = np.nonzero(index >= 0)[0]
    out["valid_index"] = np.concatenate([vi, np.full(F - len(vi), -1, np.int64)])
    out["count"] = len(vi)
    return out


def crop64(g2l, cloud, cfg, tol=TOL, sabotage=()):
    """`close_region_ref.regions64` of the view with this class's x range (the depth slab alone); the sabotaged forms
    leave out the y or z shift of the stored set (:316-317)."""
    s = cfg.search
    reg = CRR.regions64(np.asarray(g2l).astype(np.float32), cloud, s, None, tol)
    for r in reg:
        if r.get("local") is not None and ("no_y_offset" in sabotage or "no_z_offset" in sabotage):
            r["local"] = r["local"].copy()
            if "no_y_offset" in sabotage:
                r["local"][1] -= CRR._f32(s.half_bottom_space)
            if "no_z_offset" in sabotage:
                r["local"][2] -= CRR._f32(s.half_hand_thickness)
    return reg


def scene64(g2l, scene, normals, labels, cfg, tol=TOL, sabotage=(), dl=None):
    """g2l (K, 4, 4) fp32 (a zero matrix = a row that is not scanned), scene / normals (3, M) fp32, labels (M,) ->
    dict of numpy arrays of length K.  dl (K,): the depth of the taken placement, read by the sabotage "slab_at_dl"."""
    k = LR.constants(cfg.search)
    G = np.asarray(g2l, np.float32).astype(np.float64)
    P = np.asarray(scene, np.float32).astype(np.float64)
    Nn = np.asarray(normals, np.float32).astype(np.float64)
    lab = np.asarray(labels).astype(np.int64)
    K = len(G)
    out = {n: np.zeros(K, np.int64) for n in ("slab", "back", "finger", "close", "multi", "n_left", "n_right", "stage",
                                               "non_collision", "single_label", "amb_slab")}
    out.update({n: np.zeros(K) for n in ("score", "left_y", "right_y", "mean_left", "mean_right")})
    out["decided"] = np.ones(K, bool)
    out["clear"] = np.ones(K, bool)
    out["live"] = np.zeros(K, bool)
    side = lambda n, a, thr: (n - a > thr) or (n + a <= thr)          # noqa: E731
    for i in range(K):
        g = G[i]
        if not g.any() or not np.isfinite(g).all():
            continue
        out["live"][i] = True
        with np.errstate(invalid="ignore"):
            x, y, z = g[:3, :3] @ P + g[:3, 3:4]
            lo, hi = -k["bl"], k["fl"]
            if "slab_at_dl" in sabotage:
                lo, hi = lo + dl[i], hi + dl[i]
            slab = (x < hi) & (x > lo)
            near_x = LR._near(x, (lo, hi), tol)
            zin = (z < k["hht"]) & (z > -k["hht"])
            back = slab & zin & (y < k["hbw"]) & (y > -k["hbw"]) & (x < -k["m"])
            fing = slab & zin & (((y < k["hbw"]) & (y > k["hbs"])) | ((y > -k["hbw"]) & (y < -k["hbs"])))
            closer = slab & zin & (y < k["hbs"]) & (y > -k["hbs"])
            wide = (slab | near_x) & (np.abs(z) < k["hht"] + tol) & (np.abs(y) < k["hbw"] + tol)
            amb = wide & (near_x | LR._near(z, (k["hht"], -k["hht"]), tol) |
                          LR._near(y, (k["hbw"], -k["hbw"], k["hbs"], -k["hbs"]), tol) | (np.abs(x + k["m"]) < tol))
        n_slab, a_slab = int(slab.sum()), int(near_x.sum())
        nb, nf, ncl = int(back.sum()), int(fing.sum()), int(closer.sum())
        lc = lab[closer]
        multi = ncl > 0 and lc.min() != lc.max()
        out["slab"][i], out["amb_slab"][i] = n_slab, a_slab
        out["back"][i], out["finger"][i], out["close"][i], out["multi"][i] = nb, nf, ncl, multi
        out["clear"][i] = not amb.any()
        # can a point within tol of a face turn a verdict the reference reaches?  (in its order of returns)
        edge = near_x | LR._near(z, (k["hht"], -k["hht"]), tol)
        a_back = int((wide & (x < -k["m"] + tol) & (edge | LR._near(y, (k["hbw"], -k["hbw"]), tol) |
                                                      (np.abs(x + k["m"]) < tol))).sum())
        a_fing = int((wide & (edge | LR._near(y, (k["hbw"], -k["hbw"], k["hbs"], -k["hbs"]), tol))).sum())
        amb_c = wide & (np.abs(y) < k["hbs"] + tol) & (edge | LR._near(y, (k["hbs"], -k["hbs"]), tol))
        decided = (n_slab - a_slab >= k["slab_thr"]) or (n_slab + a_slab < k["slab_thr"])
        if not n_slab < k["slab_thr"]:
            decided &= side(nb, a_back, k["back_thr"])
            if not nb > k["back_thr"]:
                decided &= side(nf, a_fing, k["fing_thr"])
                if not nf > k["fing_thr"]:
                    if multi:
                        ls = lab[closer & ~amb_c]
                        decided &= bool(ls.size > 0 and ls.min() != ls.max())
                    else:
                        la = lab[closer | amb_c]
                        decided &= bool(la.size == 0 or la.min() == la.max())
                        a_close = int(amb_c.sum())
                        decided &= (ncl - a_close >= k["min_points"]) or (ncl + a_close < k["min_points"])
                        if not ncl < k["min_points"]:
                            decided &= a_close == 0           # (the extrema and the bands read every member)
        few = ncl <= k["min_points"] if "min_points_le" in sabotage else ncl < k["min_points"]
        few = few or ncl == 0
        if ncl > 0:
            out["left_y"][i], out["right_y"][i] = y[closer].max(), y[closer].min()
        collision = 2 if nb > k["back_thr"] else 3 if nf > k["fing_thr"] else 0
        if n_slab < k["slab_thr"]:
            stage = 1
        elif "labels_before_collision" in sabotage and multi:
            stage = 4
        elif collision:
            stage = collision
        elif "few_before_labels" in sabotage and few:
            stage = 6                                      # returned at the min-points line BEFORE label_bool is set
        elif multi:
            stage = 4
        elif few:
            stage = 5
        else:
            stage = 0
        nc = 0 if stage in (1, 2, 3) else 1
        sl = 1 if stage in (0, 5) else 0
        if "empty_label_0" in sabotage and stage == 5 and ncl == 0:
            sl = 0
        if stage == 6:
            stage = 5
        out["stage"][i], out["non_collision"][i], out["single_label"][i] = stage, nc, sl
        if stage == 0:
            yc = y[closer]
            ny = np.abs(g[1, :3] @ Nn[:, closer])
            ly, ry = yc.max(), yc.min()
            d = min((ly - ry) / 3, k["nd"])
            il, ir = yc > ly - d, yc < ry + d
            if "bands_swapped" in sabotage:
                il, ir = ir, il
            decided &= not ((np.abs(yc - (ly - d)) < tol) | (np.abs(yc - (ry + d)) < tol)).any()
            out["n_left"][i], out["n_right"][i] = il.sum(), ir.sum()
            with np.errstate(invalid="ignore", divide="ignore"):
                ml = ny[il].sum() / il.sum() if il.sum() else np.nan
                mr = ny[ir].sum() / ir.sum() if ir.sum() else np.nan
            out["mean_left"][i], out["mean_right"][i], out["score"][i] = ml, mr, ml * mr
        out["decided"][i] = decided
    return out


def label64(points, frames, cloud, scene, scene_normals, scene_labels, cfg, tol=TOL, sabotage=(), live=None):
    """The view search, the crop of the view and the scene grade of the taken placements -> (view dict with `regions`,
    scene dict over the same F rows)."""
    v = view64(points, frames, cloud, cfg, tol, None, live, sabotage)
    v["regions"] = crop64(v["g2l"], cloud, cfg, tol, sabotage)
    dep = cfg.search.tables()["depth"].numpy().astype(np.float64)
    T = cfg.search.shape[1]
    dl = np.where(v["index"] >= 0, dep[np.maximum(v["index"], 0) // T], 0.0)
    t = scene64(v["g2l"].astype(np.float32), scene, scene_normals, scene_labels, cfg, tol, sabotage, dl)
    return v, t


def keep_masks(v, t):
    """-> (frames (F,) bool, grasps (F,) bool): the rows an fp32 implementation is held to.  A frame is kept when the
    view stage is decided and no member of its crop is ambiguous; a grasp when its frame is kept, it was
    taken, and the scene stage is decided."""
    amb_crop = np.array([len(r["ambiguous"]) > 0 for r in v["regions"]], bool)
    kf = v["decided"] & ~amb_crop
    return kf, kf & (v["index"] >= 0) & t["decided"]


_SCENE_KEYS = ("stage", "non_collision", "single_label", "n_left", "n_right", "slab")


def altered_rows(case, name, base=None, keep=None):
    """How many kept rows of `case` = the arguments of `label64` the mistake `name` changes: frames whose placement,
    matrix or stored set differ, plus grasps (same placement on both sides) whose scene outputs differ."""
    if name in SABOTAGE_CONFIG:
        cfg = dataclasses.replace(case[6], search=dataclasses.replace(case[6].search, **SABOTAGE_CONFIG[name]))
        case, base, keep = case[:6] + (cfg,), None, None
    v0, t0 = base or label64(*case)
    v1, t1 = label64(*case, sabotage=(name,))
    kf, kg = keep or keep_masks(v0, t0)
    F = len(kf)
    df = (v0["index"] != v1["index"]) | (np.abs(v0["g2l"] - v1["g2l"]).max((1, 2)) > 1e-5)
    for f in range(F):
        if df[f] or v0["index"][f] < 0:
            continue
        c = v0["regions"][f]["certain"]
        df[f] = not np.array_equal(c, v1["regions"][f]["certain"]) or \
            (len(c) > 0 and np.abs(v0["regions"][f]["local"][:, c] - v1["regions"][f]["local"][:, c]).max() > 1e-5)
    dg = np.zeros(F, bool)
    for key in _SCENE_KEYS:
        dg |= t0[key] != t1[key]
    with np.errstate(invalid="ignore"):
        for key in ("score", "mean_left", "mean_right"):
            a, b = t0[key], t1[key]
            dg |= ~((np.abs(a - b) <= 1e-6) | (np.isnan(a) & np.isnan(b)))
    return int((df & kf).sum()) + int((dg & kg & ~df).sum())


def counts(v, t, kf, kg):
    """The cases the fixture is for, counted on its kept rows (tools/gen_golden_eval_data.py: REQUIRED)."""
    have = {name: int(((t["stage"] == i) & kg).sum()) for i, name in enumerate(STAGES)}
    have["not_first"] = int(((v["index"] > 0) & kf).sum())
    have["frame_gate"] = int(((v["flags"] == 4) & kf).sum())
    have["reach_gate"] = int(((v["flags"] == 8) & kf).sum())
    have["depth_skipped"] = int((v["depth_skipped"] & kf).sum())
    return have


def load_fixture():
    """tests/golden/eval_data.npz (tools/gen_golden_eval_data.py) as a dict, the stored maps dense: `maps`
    (len(stored_rows), 12, R, R)."""
    path = os.path.join(ROOT, "tests", "golden", "eval_data.npz")
    with np.load(path) as z:
        fx = {k: z[k] for k in z.files}
    R = int(fx["resolution"][0])
    V = len(fx["stored_rows"])
    maps = np.zeros(V * 12 * R * R, np.float32)
    maps[fx["map_nz_index"]] = fx["map_nz_value"]
    fx["maps"] = maps.reshape(V, 12, R, R)
    return fx


def case_of(fx, cfg=None):
    """The arguments of `label64` from the fixture."""
    return (fx["points"], fx["frames"], fx["cloud"], fx["scene"], fx["scene_normals"], fx["scene_labels"],
            cfg or default_config())


def lattice_case(rng, n_points, n_frames, cfg):
    """A small scene whose every VIEW row is decided, for the loop-edge tests (`precomputed_view_ref.lattice_scene` with
    an all-true mask), with normals and labels so that the same cloud serves as the dense scene of the scene stage.
    -> (points (F, 3), frames (F, 3, 3), cloud (3, N), normals (3, N) fp32, labels (N,) int32)."""
    L, T = cfg.search.shape
    vc = SimpleNamespace(search=cfg.search, valid_search_min=0.0, valid_antipodal_min=0.0)
    P, Fr, _, _, _, cloud, lab = PV.lattice_scene(rng, n_points, n_frames, vc, mask=np.ones((n_frames, L, T), bool))
    nrm = rng.standard_normal((3, n_points))
    nrm /= np.linalg.norm(nrm, axis=0, keepdims=True)
    return P, Fr, cloud, nrm.astype(np.float32), lab.astype(np.int32)
