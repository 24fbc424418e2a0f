"""Float64 yardstick of the fast baseline labels (`postprocess.grade_precomputed_baseline_frames`,
`label_precomputed_baseline_view`, csrc/precomputed_view.hip; the reference's
`TorchPrecomputedBaselinePointCloud._find_match`, `magic_formula`, `_table_collision_check` and `finger_hand`,
data_gen/pcd_classes/torch_precomputed_baseline.py:134-180,227-383).  TEST INFRASTRUCTURE ONLY.

It composes what exists: `precomputed_view_ref.match64` (stage A, with the search threshold at -inf),
`precomputed_view_ref.grade64` for the per-placement counts and gates (run WITHOUT its label gate on one label), the
fold of this class (`fold64`) and `close_region_ref.regions64` / `projection64` for the crop of the VIEW cloud.

  * `grade64`   per candidate row: `back`, `finger`, `close`, `table_collision`, `slab_count`, `scores` (the looked-up
                score where every gate passed, else 0), `index`, `score`, `valid`, `g2l` (float64), `decided`.
  * `fold64`    the first placement, depths outer and rolls inner, whose score is > 0 and > every earlier taken one.
  * `label64`   stage A, the gather of the candidate rows, `grade64`, and the crop `regions`.
  * `SABOTAGES` the mistakes a test must see; `altered_rows` counts the kept rows one of them changes.

The kernels' loop structure (what the edge shapes of tests/test_precomputed_baseline_gpu.py cross): that of
csrc/precomputed_view.hip's sweep with `PVB_SLOTS` frames per workgroup and pass, so a pass holds `FRAMES_PER_PASS`
frames."""
import dataclasses
import os
import re
from types import SimpleNamespace

import numpy as np

from tests import close_region_ref as CRR
from tests import precomputed_view_ref as PV

ROOT = PV.ROOT
FRAMES_PER_PASS = 640       # csrc/precomputed_view.hip: PV_GX * PVB_SLOTS (tests/test_precomputed_baseline_ref.py reads the source)
SABOTAGES = ("label_gate", "fold_ge", "rolls_outer", "search_threshold_50", "antipodal_f32", "flip_plain_scores",
             "x_range_baseline", "crop_scene", "normals_unoriented", "no_depth_shift", "g2l_order", "no_positive_rule")
# A mistake that the reference's constants hide is looked for with another constant.  The rule "score > 0" (:339 against
# the zeroed slot :119) cannot show while the mask asks for a score above 0.3: it is looked for with the threshold at -1,
# where every matched placement is open and a placement that passes with the score 0 must still not be taken.
SABOTAGE_CONFIG = {"no_positive_rule": {"antipodal_threshold": -1.0}}
# `<=` at the min-points gate (:333) is a mistake `grade64` can make ("min_points_le"), but no fixture row sees it: it
# takes a placement that passes every other gate with exactly CLOSE_REGION_MIN_POINTS points between the fingers.


def slots_in_source():
    """(PV_GX, PVB_SLOTS) as csrc/precomputed_view.hip compiles them."""
    text = open(os.path.join(ROOT, "s4g_release_amd", "csrc", "precomputed_view.hip")).read()
    gx = int(re.search(r"constexpr int PV_GX = (\d+);", text).group(1))
    slots = int(re.search(r"constexpr int PVB_SLOTS = (\d+);", text).group(1))
    return gx, slots


def default_config(**kw):
    from s4g_release_amd.postprocess import PrecomputedBaselineConfig
    return PrecomputedBaselineConfig(**kw)


def view_cfg(cfg, sabotage=()):
    """What `precomputed_view_ref` reads of a config: the search threshold is off (-inf: every int64 score is above)."""
    return SimpleNamespace(search_threshold=50.0 if "search_threshold_50" in sabotage else -np.inf,
                           antipodal_threshold=cfg.antipodal_threshold, region=cfg.view_config().region,
                           search=cfg.search, valid_search_min=0.0, valid_antipodal_min=0.0)


def fold64(scores, L, T, sabotage=()):
    """scores (L, T) fp32 -> (index, score): :337-348.  A NaN is never taken."""
    best, bi = 0.0, -1
    if "no_positive_rule" in sabotage:
        best = -np.inf
    order = [(d, t) for t in range(T) for d in range(L)] if "rolls_outer" in sabotage else \
        [(d, t) for d in range(L) for t in range(T)]
    for d, t in order:
        v = float(scores[d, t])
        take = (v >= best and v > 0) if "fold_ge" in sabotage else v > best
        if take:
            best, bi = v, d * T + t
    return bi, (best if bi >= 0 else 0.0)


def g2l64(point, frame, search, index, sabotage=()):
    """LOCAL_TO_LOCAL_SEARCH[index] @ [R^T | -R^T p] in float64 (4, 4); zeros for index -1."""
    if index < 0:
        return np.zeros((4, 4))
    tb = search.tables()
    T = search.shape[1]
    dep, cs, sn = (tb[k].numpy().astype(np.float64) for k in ("depth", "cos", "sin"))
    R, p = np.asarray(frame, np.float32).astype(np.float64), np.asarray(point, np.float32).astype(np.float64)
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = R.T, -(R.T @ p)
    S = np.eye(4)
    d, t = divmod(int(index), T)
    if "no_depth_shift" not in sabotage:
        S[0, 3] = -dep[d]
    S[1, 1], S[1, 2], S[2, 1], S[2, 2] = cs[t], sn[t], -sn[t], cs[t]
    return G @ S if "g2l_order" in sabotage else S @ G


def grade64(points, frames, mask, pre_antipodal, cloud, cfg, tol=4e-6, frame_count=None, sabotage=(), labels=None):
    """points (F, 3), frames (F, 3, 3), mask / pre_antipodal (F, L, T), cloud (3, M) fp32 -> dict of numpy arrays.
    `labels` (M,) is read by the sabotage "label_gate" only."""
    s = cfg.search
    L, T = s.shape
    F = len(points)
    M = np.asarray(cloud).shape[1]
    gate = "label_gate" in sabotage and labels is not None
    lab = np.asarray(labels) if gate else np.zeros(M, np.int64)
    vc = view_cfg(cfg)
    if "min_points_le" in sabotage:           # `<=` where the reference has `<` (:333): one more point is asked for
        vc.search = dataclasses.replace(s, close_region_min_points=s.close_region_min_points + 1)
    y = PV.grade64(points, frames, mask, np.zeros((F, L, T), np.int64), pre_antipodal, cloud, lab, vc, tol, frame_count,
                   () if gate else ("no_label_gate",))
    out = {k: y[k] for k in ("back", "finger", "close", "table_collision", "slab_count", "amb_slab", "clear", "reason",
                             "gate", "decided")}
    out["scores"] = y["antipodal_score"]
    out["index"] = np.full(F, -1, np.int64)
    out["score"] = np.zeros(F, np.float32)
    out["g2l"] = np.zeros((F, 4, 4))
    out["first_pass"] = np.full(F, -1, np.int64)
    out["tie"] = np.zeros(F, bool)
    for f in range(F):
        sc = out["scores"][f]
        passed = np.nonzero((y["reason"][f] == 0).reshape(-1))[0]
        out["index"][f], out["score"][f] = fold64(sc, L, T, sabotage)
        if len(passed):
            out["first_pass"][f] = passed[0]
            top = sc.reshape(-1)[passed]
            out["tie"][f] = (top == top.max()).sum() >= 2
        out["g2l"][f] = g2l64(points[f], frames[f], s, out["index"][f], sabotage)
    out["valid"] = out["index"] >= 0
    vi = np.nonzero(out["valid"])[0]
    out["valid_index"] = np.concatenate([vi, np.full(F - len(vi), -1, np.int64)])
    out["count"] = len(vi)
    return out


def x_range(cfg, sabotage=()):
    s = cfg.search
    return (-s.bottom_length, s.finger_length) if "x_range_baseline" in sabotage else (0.0, s.finger_length)


def label64(reference_cloud, cloud, scene, camera, cfg, radius, tol=4e-6, sabotage=()):
    """The whole call on one scene -> (match dict, grade dict over the `frame_count` candidate rows with `regions`:
    `close_region_ref.regions64` of the view cloud per row, and `normals32` the normals the crop reads)."""
    msab = tuple(x for x in sabotage if x in ("antipodal_f32", "flip_plain_scores"))
    m = PV.match64(reference_cloud, cloud, scene, camera, view_cfg(cfg, sabotage), radius, msab)
    pts, frm, mask, _, pa = PV.gather_rows(m, cloud)
    g = grade64(pts, frm, mask, pa, scene["points"], cfg, tol, None, sabotage, scene.get("labels"))
    g["cloud_index"] = m["frame_index"][:m["frame_count"]][g["valid_index"][:g["count"]]]
    crop = scene["points"] if "crop_scene" in sabotage else cloud
    g["regions"] = CRR.regions64(g["g2l"].astype(np.float32), crop, cfg.search, x_range(cfg, sabotage), tol)
    if "crop_scene" in sabotage:
        g["normals32"] = np.asarray(scene["normals"], np.float32)
    elif "normals_unoriented" in sabotage:
        idx = m["nearest"]
        n = np.where(idx[None] >= 0, np.asarray(scene["normals"], np.float64)[:, np.maximum(idx, 0)],
                     np.array([[0.0], [0.0], [1.0]]))
        g["normals32"] = (n / np.sqrt((n * n).sum(0))).astype(np.float32)
    else:
        g["normals32"] = m["normals"].T.astype(np.float32)
    return m, g


def decided(m, g):
    """-> (view points (N,) bool, frame rows (F,) bool), as `precomputed_view_ref.decided`."""
    return PV.decided(m, g)


def ambiguous_crop(g, rows=None):
    """(F,) bool: the rows whose crop holds a member within `tol` of a face."""
    rows = range(len(g["regions"])) if rows is None else rows
    return np.array([len(g["regions"][r]["ambiguous"]) > 0 for r in rows], bool)


def altered_rows(case, name, base=None):
    """How many kept rows of `case` = (reference_cloud, cloud, scene, camera, cfg, radius) the mistake `name` changes:
    view points whose scores, mask or candidacy differ, plus candidate frames (compared by view point) whose index,
    score, matrix, per-placement outputs, crop members or crop normals differ or which exist on one side only."""
    if name in SABOTAGE_CONFIG:
        case = case[:4] + (dataclasses.replace(case[4], **SABOTAGE_CONFIG[name]),) + case[5:]
        base = None
    m0, g0 = base or label64(*case)
    m1, g1 = label64(*case, sabotage=(name,))
    kp, kf = decided(m0, g0)
    dp = (m0["pre_antipodal"] != m1["pre_antipodal"]).any((1, 2)) | (m0["mask"] != m1["mask"]).any((1, 2)) | \
        (m0["candidate"] != m1["candidate"])
    row1 = {int(v): r for r, v in enumerate(m1["frame_index"][:m1["frame_count"]])}
    df = np.zeros(m0["frame_count"], bool)
    for r, v in enumerate(m0["frame_index"][:m0["frame_count"]]):
        r1 = row1.get(int(v))
        if r1 is None:
            df[r] = True
            continue
        df[r] = g0["index"][r] != g1["index"][r1] or g0["score"][r] != g1["score"][r1] or \
            np.abs(g0["g2l"][r] - g1["g2l"][r1]).max() > 1e-5 or \
            not np.array_equal(g0["scores"][r], g1["scores"][r1]) or \
            not np.array_equal(g0["regions"][r]["certain"], g1["regions"][r1]["certain"])
        if not df[r] and g0["index"][r] >= 0:
            c = g0["regions"][r]["certain"]
            df[r] = len(c) > 0 and np.abs(g0["normals32"][:, c] - g1["normals32"][:, c]).max() > 1e-6 \
                if g0["normals32"].shape == g1["normals32"].shape else True
    return int((dp & kp).sum()) + int((df & kf).sum())


def load_fixture():
    """tests/golden/precomputed_baseline.npz (tools/gen_golden_precomputed_baseline.py) as a dict, the stored maps dense:
    `maps` (len(stored_rows), 12, R, R)."""
    path = os.path.join(ROOT, "tests", "golden", "precomputed_baseline.npz")
    with np.load(path) as z:
        fx = {k: z[k] for k in z.files}
    R = int(fx["resolution"][0])
    maps = np.zeros(len(fx["stored_rows"]) * 12 * R * R, np.float32)
    maps[fx["map_nz_index"]] = fx["map_nz_value"]
    fx["maps"] = maps.reshape(-1, 12, R, R)
    return fx


def case_of(fx, cfg=None):
    """(reference_cloud, cloud, scene, camera, cfg, radius) of the fixture: the arguments of `label64`."""
    return (fx["reference_cloud"], fx["cloud"], PV.scene_of(fx), fx["camera"], cfg or default_config(),
            float(fx["radius"][0]))


def counts(fx, m, g):
    """The cases the fixture is for, counted on its kept rows (tools/gen_golden_precomputed_baseline.py: REQUIRED)."""
    kp, kf = fx["keep_points"].astype(bool), fx["keep_frames"].astype(bool)
    pts, frm, mask, _, pa = PV.gather_rows(m, fx["cloud"])
    gated = grade64(pts, frm, mask, pa, fx["scene"], default_config(), sabotage=("label_gate",), labels=fx["labels"])
    best_reason = np.array([gated["reason"][f].reshape(-1)[g["index"][f]] if g["index"][f] >= 0 else -1
                            for f in range(len(kf))])
    vk = g["valid"] & kf
    cand = m["candidate"] & kp
    have = {"valid": int(vk.sum()), "valid_two_labels": int((vk & (best_reason == 6)).sum()),
            "not_first": int((vk & (g["index"] != g["first_pass"])).sum()), "tie": int((vk & g["tie"]).sum()),
            "flipped": int((m["flipped"] & cand).sum()), "unflipped": int((~m["flipped"] & cand).sum()),
            "unmatched": int(((m["nearest"] < 0) & kp).sum()), "region_only": int((m["region_only"] & kp).sum())}
    reason = g["reason"][kf]
    for i, name in enumerate(PV.REASONS):
        have[name] = int((reason == i).sum())
    return have


REQUIRED = {"valid": 40, "valid_two_labels": 20, "not_first": 20, "tie": 20, "table": 20, "slab": 20, "back": 20,
            "finger": 20, "few": 20, "masked": 20, "masked_depth": 20, "flipped": 100, "unflipped": 100, "unmatched": 10,
            "region_only": 20}
