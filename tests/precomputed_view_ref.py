"""Float64 yardstick of the fast pipeline's view stage (`postprocess.match_scene_frames`, `grade_precomputed_frames`,
`label_precomputed_view`, csrc/precomputed_view.hip; the reference's `TorchPrecomputedSingleViewPointCloud._find_match`,
`magic_formula`, `_table_collision_check` and `finger_hand`,
data_gen/pcd_classes/torch_precomputed_single_view_point_cloud.py:130-185,258-396).  TEST INFRASTRUCTURE ONLY.

  * `match64`   stage A per view point from the fp32 inputs: the nearest scene point (`contact_search_ref.nearest`), the
                normal in double, the flip, the frame, the scores, the mask, the candidates in ascending order; `near`
                (a neighbour at the radius or a tie within fp32 error) and `graze` (|n . x| < 1e-6) are what `decided`
                reads.
  * `grade64`   stage B per candidate row on freshly zeroed results (decision "no stale slots"): exact products of the
                fp32 inputs and of the fp32 cos / sin the reference forms; per frame whether it is DECIDED at `tol`:
                no point within `tol` of a face, slab bound or margin could turn a verdict, and no table corner lies
                within `tol` of the limit.  `reason` says why a placement was not scored (`REASONS`).
  * `label64`   both, with the gather of the candidate rows between them.
  * `decided`   -> (view points, frame rows) an fp32 implementation is held to.
  * `SABOTAGES` the mistakes the fixture must see; `altered_rows` counts the kept rows one of them changes.
  * `lattice_scene`  a scene whose every row is decided, for the loop-edge tests.

The kernels' loop structure (what the edge shapes of tests/test_precomputed_view_gpu.py cross): point chunks per scene =
ceil(M / 16 384) within [4, 64] (empty below M = 4); sweeps of 1 024 points; 32 workgroups share a scene's frames,
`PV_SLOTS` frames per workgroup and pass, so a pass holds `FRAMES_PER_PASS` frames."""
import os
import re

import numpy as np

from tests import contact_search_ref as CR
from tests import local_search_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES_PER_PASS = 384       # csrc/precomputed_view.hip: PV_GX * PV_SLOTS (tests/test_precomputed_view_ref.py reads the source)
REASONS = ("scored", "table", "slab", "back", "finger", "few", "labels", "frame", "masked", "masked_depth")
GRAZE = 1e-6
REQUIRED = {"valid": 40, "flipped": 100, "unflipped": 100, "unmatched": 10, "region_only": 20, "table": 20, "slab": 20,
            "back": 20, "finger": 20, "few": 20, "labels": 20, "masked": 20, "masked_depth": 20, "reach": 20,
            "reach_valid": 10}
SCENE_KEYS = ("points", "normals", "labels", "frames", "search_score", "inv_search_score", "antipodal_score",
              "inv_antipodal_score")


def frames_per_pass_in_source():
    """PV_GX * PV_SLOTS as csrc/precomputed_view.hip compiles them."""
    text = open(os.path.join(ROOT, "s4g_release_amd", "csrc", "precomputed_view.hip")).read()
    gx = int(re.search(r"constexpr int PV_GX = (\d+);", text).group(1))
    slots = int(re.search(r"constexpr int PV_SLOTS = (\d+);", text).group(1))
    return gx * slots


def default_config(**kw):
    from s4g_release_amd.postprocess import PrecomputedViewConfig
    return PrecomputedViewConfig(**kw)


def match64(reference_cloud, cloud, scene, camera, cfg, radius, sabotage=()):
    """reference_cloud, cloud (3, N) fp32; scene: dict of `SCENE_KEYS` (points, normals (3, M), frames (M, 3, 3), the
    four scores (M, L, T)); camera (3,) -> dict of numpy arrays per view point."""
    q = np.asarray(cloud, np.float32).astype(np.float64).T
    qr = np.asarray(reference_cloud, np.float32).astype(np.float64).T
    nrm = np.asarray(scene["normals"], np.float32).astype(np.float64).T
    cam = np.asarray(camera, np.float32).astype(np.float64)
    fr = np.asarray(scene["frames"], np.float32).astype(np.float64)
    N = len(q)
    L, T = scene["search_score"].shape[1:]
    idx, near = CR.nearest(cloud if "match_noisy" in sabotage else reference_cloud, scene["points"], radius)
    idx = idx.copy()
    idx[~np.isfinite(q).all(1)] = -1
    out = {"nearest": idx, "near": near, "normals": np.zeros((N, 3)), "flipped": np.zeros(N, bool),
           "graze": np.zeros(N, bool), "frames": np.tile(np.eye(3), (N, 1, 1)),
           "pre_search": np.zeros((N, L, T), np.int64), "pre_antipodal": np.zeros((N, L, T), np.float32)}
    origin = qr if "orient_reference" in sabotage else q
    for j in range(N):
        i = int(idx[j])
        n = np.array([0.0, 0.0, 1.0])
        if i >= 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                n = nrm[i] / np.sqrt((nrm[i] * nrm[i]).sum())                    # normalize_normals (:158)
        with np.errstate(invalid="ignore", over="ignore"):
            ref = cam - origin[j]
        if np.isfinite(ref).all():                                               # :159
            if not np.isnan(n).any() and not n.any():
                rl = float(np.sqrt((ref * ref).sum()))
                n = ref / rl if rl > 0.0 else np.array([0.0, 0.0, 1.0])
            elif float(n[0] * ref[0] + n[1] * ref[1] + n[2] * ref[2]) < 0.0:
                n = -n
        out["normals"][j] = n
        if i < 0:
            continue
        R = fr[i].copy()
        dot = float(n[0] * R[0, 0] + n[1] * R[1, 0] + n[2] * R[2, 0])            # :163
        flip = dot > 0
        out["graze"][j] = abs(dot) < GRAZE
        out["flipped"][j] = flip
        if flip and "no_flip" not in sabotage:
            R[:, 0:3 if "flip_all_columns" in sabotage else 2] *= -1             # :166
        out["frames"][j] = R
        inv = flip                                                               # :167-170
        if "flip_plain_scores" in sabotage:
            inv = False
        if "inv_without_flip" in sabotage:
            inv = True
        out["pre_search"][j] = scene["inv_search_score" if inv else "search_score"][i]
        out["pre_antipodal"][j] = scene["inv_antipodal_score" if inv else "antipodal_score"][i]
    ps, pa = out["pre_search"].astype(np.float64), out["pre_antipodal"]
    st, at = float(cfg.search_threshold), float(cfg.antipodal_threshold)
    sb = ps >= st if "ge_thresholds" in sabotage else ps > st                    # :181
    if "antipodal_f32" in sabotage:
        ab = pa > np.float32(at)
    elif "ge_thresholds" in sabotage:
        ab = pa.astype(np.float64) >= at
    else:
        ab = pa.astype(np.float64) > at                                          # :182, float64 as numpy compares
    mask = sb & ab
    if "mask_ignored" in sabotage:
        mask = np.broadcast_to((idx >= 0)[:, None, None], mask.shape).copy()
    out["mask"] = mask
    z = np.asarray(reference_cloud if "region_reference_z" in sabotage else cloud, np.float32)[2]
    with np.errstate(invalid="ignore"):
        above = z > np.float32(cfg.region)                                       # :173, fp32
    out["candidate"] = (idx >= 0) & mask.any((1, 2)) & above
    out["region_only"] = (idx >= 0) & mask.any((1, 2)) & ~above
    fi = np.nonzero(out["candidate"])[0]
    out["frame_index"] = np.concatenate([fi, np.full(N - len(fi), -1, np.int64)]).astype(np.int32)
    out["frame_count"] = len(fi)
    return out


def grade64(points, frames, mask, pre_search, pre_antipodal, cloud, labels, cfg, tol=4e-6, frame_count=None,
            sabotage=()):
    """points (F, 3), frames (F, 3, 3), mask / pre_search / pre_antipodal (F, L, T), cloud (3, M) fp32, labels (M,) ->
    dict of numpy arrays: (F, L, T) `search_score`, `objects_label`, `back`, `finger`, `close` (int64),
    `table_collision` (bool), `antipodal_score` (float32), `reason` (index into REASONS); (F, L) `slab_count`; (F,)
    `valid`, `gate`, `decided`; `valid_index` (F,) ascending, -1 padded; `count`."""
    s = cfg.search
    k = LR.constants(s)
    L, T = s.shape
    F = len(points)
    n_live = F if frame_count is None else max(0, min(F, int(frame_count)))
    P = np.asarray(cloud, np.float32).astype(np.float64)
    lab = np.asarray(labels).astype(np.int64)
    mask = np.asarray(mask, bool).reshape(F, L, T).copy()
    if "mask_ignored" in sabotage:
        mask[:] = True
    ps = np.asarray(pre_search).reshape(F, L, T).astype(np.int64)
    pa = np.asarray(pre_antipodal, np.float32).reshape(F, L, T)
    out = {n: np.zeros((F, L, T), np.int64) for n in ("search_score", "back", "finger", "close")}
    out["objects_label"] = np.full((F, L, T), s.no_label, np.int64)
    out["table_collision"] = np.zeros((F, L, T), bool)
    out["antipodal_score"] = np.zeros((F, L, T), np.float32)
    out["reason"] = np.full((F, L, T), 7, np.int64)
    out["clear"] = np.ones((F, L, T), bool)
    out["slab_count"] = np.zeros((F, L), np.int64)
    out["amb_slab"] = np.zeros((F, L), np.int64)
    out["valid"] = np.zeros(F, bool)
    out["gate"] = np.zeros(F, bool)
    out["reach"] = np.zeros(F, bool)
    out["decided"] = np.ones(F, bool)
    corners = np.array([[x, y, z] for x in (k["fl"], -k["bl"]) for y in (k["hbw"], -k["hbw"]) for z in (k["hht"], -k["hht"])])
    r2lim = (k["hbw"] ** 2 + k["hht"] ** 2) * 1.01 + 1e-6
    vs_min, va_min = float(np.float32(cfg.valid_search_min)), float(np.float32(cfg.valid_antipodal_min))
    side = lambda n, a, thr: (n - a > thr) or (n + a <= thr)          # noqa: E731
    for f in range(n_live):
        R = np.asarray(frames[f], np.float32).astype(np.float64)
        p = np.asarray(points[f], np.float32).astype(np.float64)
        if not (np.isfinite(R).all() and np.isfinite(p).all()):
            out["decided"][f] = False
            continue
        mean = np.abs(R).mean()
        if abs(mean - 1e-6) < 1e-8:
            out["decided"][f] = False
        if mean < 1e-6:                                                          # :295
            continue
        reach = p[2] + R[2, 0] * k["fl"] < k["th"]        # what grade_local_search's second gate would reject
        out["reach"][f] = reach
        if reach and "reach_gate" in sabotage:
            continue
        out["gate"][f] = True
        decided = True
        table = np.zeros((L, T), bool)
        for d in range(L):                                                       # :258-275
            for t in range(T):
                c, sn = k["cos"][t], k["sin"][t]
                m = np.array([R[2, 0], R[2, 1] * c + R[2, 2] * sn, -R[2, 1] * sn + R[2, 2] * c])
                zc = corners @ m + (R[2, 0] * k["depth"][d] + p[2])
                table[d, t] = (zc < k["tl"]).any()
                if mask[f, d, t]:
                    decided &= not (np.abs(zc - k["tl"]) < tol).any()
        out["table_collision"][f] = table
        if "no_table" in sabotage:
            table = np.zeros((L, T), bool)
        mk = mask[f]
        out["reason"][f] = np.where(mk, 7, 8)
        if mk.any():
            with np.errstate(invalid="ignore"):
                loc = R.T @ P + (-(R.T @ p))[:, None]                            # :121-123, :301
                x, y, z = loc
                depths = [d for d in range(L) if mk[d].any()]                    # :305
                near_x = {d: (np.abs(x - k["lo"][d]) < tol) | (np.abs(x - k["hi"][d]) < tol) for d in depths}
                slab = {d: (x < k["hi"][d]) & (x > k["lo"][d]) for d in depths}  # :309-310
                keep = np.zeros(x.shape, bool)
                for d in depths:
                    keep |= slab[d] | near_x[d]
                keep &= y * y + z * z < r2lim
            slab_skip = {}
            for d in range(L):
                if d not in slab:
                    out["reason"][f, d] = 9
                    continue
                n_slab, a_slab = int(slab[d].sum()), int(near_x[d].sum())
                out["slab_count"][f, d] = n_slab
                out["amb_slab"][f, d] = a_slab
                slab_skip[d] = n_slab < k["slab_thr"]                            # :312
                decided &= (n_slab - a_slab >= k["slab_thr"]) or (n_slab + a_slab < k["slab_thr"])
            xk, yk, zk, lb = x[keep], y[keep], z[keep], lab[keep]
            for t in range(T):
                if not mk[:, t].any():
                    continue
                c, sn = k["cos"][t], k["sin"][t]
                yy, zz = c * yk + sn * zk, -sn * yk + c * zk                     # config.py:79-82
                zin = (zz < k["hht"]) & (zz > -k["hht"])
                wide_yz = (np.abs(zz) < k["hht"] + tol) & (np.abs(yy) < k["hbw"] + tol)
                near_z = LR._near(zz, (k["hht"], -k["hht"]), tol)
                for d in depths:
                    if not mk[d, t]:
                        continue
                    if table[d, t]:                                              # :327
                        out["reason"][f, d, t] = 1
                        continue
                    xs = xk - k["depth"][d]
                    sl, nx = slab[d][keep], near_x[d][keep]
                    back = sl & zin & (yy < k["hbw"]) & (yy > -k["hbw"]) & (xs < -k["m"])     # :337-340
                    fing = sl & zin & (((yy < k["hbw"]) & (yy > k["hbs"])) | ((yy > -k["hbw"]) & (yy < -k["hbs"])))
                    closer = sl & zin & (yy < k["hbs"]) & (yy > -k["hbs"])                    # :357-359
                    wide = (sl | nx) & wide_yz
                    edge = nx | near_z
                    a_back = int((wide & (xs < -k["m"] + tol) & (edge | LR._near(yy, (k["hbw"], -k["hbw"]), tol)
                                                                 | (np.abs(xs + k["m"]) < tol))).sum())
                    a_fing = int((wide & (edge | LR._near(yy, (k["hbw"], -k["hbw"], k["hbs"], -k["hbs"]), tol))).sum())
                    amb_c = wide & (np.abs(yy) < k["hbs"] + tol) & (edge | LR._near(yy, (k["hbs"], -k["hbs"]), tol))
                    a_close = int(amb_c.sum())
                    nb, nf, ncl = int(back.sum()), int(fing.sum()), int(closer.sum())
                    out["back"][f, d, t], out["finger"][f, d, t], out["close"][f, d, t] = nb, nf, ncl
                    out["clear"][f, d, t] = a_back + a_fing + a_close == 0
                    if slab_skip[d]:
                        out["reason"][f, d, t] = 2
                        continue
                    decided &= side(nb, a_back, k["back_thr"])
                    if nb > k["back_thr"]:                                       # :342
                        out["reason"][f, d, t] = 3
                        continue
                    decided &= side(nf, a_fing, k["fing_thr"])
                    if nf > k["fing_thr"]:                                       # :353
                        out["reason"][f, d, t] = 4
                        continue
                    decided &= (ncl - a_close >= k["min_points"]) or (ncl + a_close < k["min_points"])
                    if ncl < k["min_points"] or ncl == 0:                        # :363
                        out["reason"][f, d, t] = 5
                        continue
                    lc = lb[closer]
                    if lc.min() != lc.max() and "no_label_gate" not in sabotage:  # :367-371
                        out["reason"][f, d, t] = 6
                        ls = lb[closer & ~amb_c]
                        decided &= bool(ls.size > 0 and ls.min() != ls.max())
                        continue
                    la = lb[closer | amb_c]
                    decided &= bool(la.min() == la.max())
                    out["reason"][f, d, t] = 0
                    out["search_score"][f, d, t] = ps[f, d, t]                   # :373-375
                    out["objects_label"][f, d, t] = lc[0] if "no_label_gate" in sabotage else lc.min()
                    out["antipodal_score"][f, d, t] = pa[f, d, t]                # :379-381
        sc = out["antipodal_score"][f].astype(np.float64)
        with np.errstate(invalid="ignore"):
            bad = (out["search_score"][f].max() < vs_min) or (not np.isnan(sc).any() and sc.max() < va_min)   # :384
        out["valid"][f] = not bad
        out["decided"][f] &= bool(decided)
    vi = np.nonzero(out["valid"])[0]
    out["valid_index"] = np.concatenate([vi, np.full(F - len(vi), -1, np.int64)])
    out["count"] = len(vi)
    return out


def gather_rows(m, cloud, sabotage=(), scene_points=None):
    """The candidate rows of `match64`'s result: -> (points (F, 3) fp32, frames fp32, mask, pre_search, pre_antipodal)."""
    fi = m["frame_index"][:m["frame_count"]].astype(np.int64)
    pts = np.asarray(cloud, np.float32).T[fi]
    if "origin_scene_point" in sabotage:
        pts = np.asarray(scene_points, np.float32).T[m["nearest"][fi]]
    si = np.arange(len(fi)) if "scores_by_view_index" in sabotage else fi
    return (pts, m["frames"][fi].astype(np.float32), m["mask"][fi], m["pre_search"][si], m["pre_antipodal"][si])


def label64(reference_cloud, cloud, scene, camera, cfg, radius, tol=4e-6, sabotage=()):
    """Both stages on one scene -> (match dict, grade dict over the `frame_count` candidate rows)."""
    m = match64(reference_cloud, cloud, scene, camera, cfg, radius, sabotage)
    rows = gather_rows(m, cloud, sabotage, scene["points"])
    g = grade64(*rows, scene["points"], scene["labels"], cfg, tol, None, sabotage)
    g["cloud_index"] = m["frame_index"][:m["frame_count"]][g["valid_index"][:g["count"]]]
    return m, g


def decided(m, g):
    """-> (view points (N,) bool, frame rows (F,) bool): a view point is undecided where a neighbour lies at the radius,
    two neighbours tie within fp32 error or n . x lies within 1e-6 of 0; a frame row where `grade64` says so or its
    view point is undecided."""
    kp = ~m["near"] & ~m["graze"]
    fi = m["frame_index"][:m["frame_count"]].astype(np.int64)
    return kp, g["decided"] & kp[fi]


SABOTAGES = ("mask_ignored", "ge_thresholds", "antipodal_f32", "no_flip", "flip_plain_scores",
             "inv_without_flip", "flip_all_columns", "orient_reference", "match_noisy", "origin_scene_point",
             "region_reference_z", "reach_gate", "no_label_gate", "no_table", "scores_by_view_index")
_ROW_KEYS = ("search_score", "objects_label", "back", "finger", "close", "table_collision", "antipodal_score")


def scene_of(fx):
    """The scene dict of the fixture's arrays: frames and scores are stored for the matched scene points only."""
    M = fx["scene"].shape[1]
    L, T = fx["rows_search"].shape[1:]
    at = fx["rows_index"].astype(np.int64)
    sc = {"points": fx["scene"], "normals": fx["scene_normals"], "labels": fx["labels"],
          "frames": np.tile(np.eye(3, dtype=np.float32), (M, 1, 1))}
    sc["frames"][at] = fx["rows_frames"]
    for name, dt in (("search_score", np.int32), ("inv_search_score", np.int32), ("antipodal_score", np.float32),
                     ("inv_antipodal_score", np.float32)):
        sc[name] = np.zeros((M, L, T), dt)
        sc[name][at] = fx["rows_" + name.replace("_score", "")]
    return sc


def altered_rows(fx, name, base=None, cfg=None):
    """How many kept rows of the fixture `fx` the mistake `name` changes: view points whose nearest index, normal,
    flip, frame, scores, mask or candidacy differ, plus candidate frames (compared by view point) whose outputs or
    validity differ or which exist on one side only."""
    cfg = cfg or default_config()
    args = (fx["reference_cloud"], fx["cloud"], scene_of(fx), fx["camera"], cfg, float(fx["radius"][0]))
    m0, g0 = base or label64(*args)
    m1, g1 = label64(*args, sabotage=(name,))
    kp, kf = fx["keep_points"].astype(bool), fx["keep_frames"].astype(bool)
    with np.errstate(invalid="ignore"):
        dp = (m0["nearest"] != m1["nearest"]) | (np.abs(m0["normals"] - m1["normals"]).max(1) > 1e-6) | \
             (m0["flipped"] != m1["flipped"]) | (np.abs(m0["frames"] - m1["frames"]).max((1, 2)) > 0) | \
             (m0["pre_search"] != m1["pre_search"]).any((1, 2)) | (m0["pre_antipodal"] != m1["pre_antipodal"]).any((1, 2)) | \
             (m0["mask"] != m1["mask"]).any((1, 2)) | (m0["candidate"] != m1["candidate"])
    row1 = {int(v): r for r, v in enumerate(m1["frame_index"][:m1["frame_count"]])}
    df = np.zeros(m0["frame_count"], bool)
    for r, v in enumerate(m0["frame_index"][:m0["frame_count"]]):
        r1 = row1.get(int(v))
        if r1 is None:
            df[r] = True
            continue
        df[r] = bool(g0["valid"][r] != g1["valid"][r1]) or any(
            not np.array_equal(g0[key][r], g1[key][r1]) for key in _ROW_KEYS + ("slab_count",))
    return int((dp & kp).sum()) + int((df & kf).sum())


def _small_turn(rng, angle):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = rng.uniform(0, angle)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def lattice_scene(rng, n_points, n_frames, cfg, mask=None, keep_rows=(), nan_from=None):
    """A scene whose every frame row is DECIDED, for the loop-edge tests: `local_search_ref.blob_scene` (a blob between
    the fingers of a base grasp 30 cm above the table, clutter around it, the rest of the points on the table), a
    random mask with whole depths and whole frames cleared (or the caller's `mask`), synthetic scores; the points from
    `nan_from` on become NaN padding.  A frame that `grade64` calls undecided -- some point within 4e-6 of a face whose
    verdict it could turn -- is drawn again (another small turn of the base frame, another origin) until none is left;
    the rows `keep_rows` are left as the caller will overwrite them.  The choice reads the yardstick alone.
    -> (points (F, 3), frames (F, 3, 3), mask (F, L, T) bool, pre_search (F, L, T) int32, pre_antipodal (F, L, T) fp32,
    cloud (3, M) fp32, labels (M,) int32)."""
    L, T = cfg.search.shape
    P, Fr, cloud, _, lab = LR.blob_scene(rng, n_points, n_frames, cfg.search)
    if nan_from is not None:
        cloud[:, nan_from:] = np.nan
    if mask is None:
        mask = rng.random((n_frames, L, T)) < 0.6
        mask[rng.random((n_frames, L)) < 0.2] = False
        if n_frames > 2:
            mask[rng.integers(n_frames)] = False
    ps = rng.integers(0, 200, (n_frames, L, T)).astype(np.int32)
    pa = rng.uniform(0.0, 1.0, (n_frames, L, T)).astype(np.float32)
    base_R, base_p = Fr[0].astype(np.float64), P[0].astype(np.float64)
    todo = np.array([f for f in range(n_frames) if f not in keep_rows], int)
    for _ in range(40):
        if not len(todo):
            break
        y = grade64(P[todo], Fr[todo], mask[todo], ps[todo], pa[todo], cloud, lab, cfg)
        todo = todo[~y["decided"]]
        for f in todo:
            Fr[f] = (_small_turn(rng, 0.2) @ base_R).astype(np.float32)
            P[f] = (base_p + rng.uniform(-0.005, 0.005, 3)).astype(np.float32)
    assert not len(todo), "no decided frame found for rows %s" % todo
    return P, Fr, mask, ps, pa, cloud, lab
