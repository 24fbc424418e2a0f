"""Float64 yardstick of the contact model's label path (`postprocess.grade_contact_frames`, `match_nearest`,
`label_contact_view`; csrc/contact_search.hip): the reference's `TorchPrecomputedSingleViewPointCloud.finger_hand`,
`_table_collision_check`, `_find_match` and `run_score` (data_gen/pcd_classes/torch_contact_single_view_point_cloud.py)
restated in numpy on one scene.  `dtype=np.float32` gives the literal fp32 restatement: the same steps with every
operation rounded to fp32, in the order the kernels use.

The fp32 inputs are taken as exact; the bounds are the fp32 values the reference compares against (a Python float
rounded once).  `decided` marks the rows an fp32 implementation is held to:
  frames        no scene point within TOL = 1e-6 m of a boundary of a region it would otherwise be in, no gripper
                corner within TOL of the table plane;
  view points   the nearest and second-nearest squared distances differ by at least 4 fp32 ulp, no scene point is
                that close to the radius, and the best two valid scores differ by at least 1e-6 relative unless their
                inputs are bit-equal.

`sabotage`: names of deliberate mistakes (tests/test_contact_search_ref.py shows the fixture sees each of them)."""
import numpy as np

TOL = 1e-6
FAIL_TABLE, FAIL_FINGER, FAIL_BEHIND, FAIL_LABELS, FAIL_EMPTY, FAIL_NONFINITE = 1, 2, 4, 8, 16, 32
ULP4 = 4.0 * 2.0 ** -23


class Config:
    """The reference's constants (torch_contact_single_view_point_cloud.py:11-15, configs/config.py:17,40,50-56,89),
    written out here so that the yardstick does not read the package under test."""
    width_search = (-0.005, 0.005, 0)
    height_search = (-0.005, 0.005, 0)
    length_search = (0,)
    table_height = 0.75
    table_collision_offset = 0.005
    back_collision_margin = 0.0
    half_bottom_width = 0.057
    bottom_length = 0.08
    finger_width = 0.023
    half_hand_thickness = 0.012
    finger_length = 0.09
    no_label = 122

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def half_bottom_space(self):
        return self.half_bottom_width - self.finger_width

    @property
    def placements(self):
        return len(self.height_search) * len(self.width_search) * len(self.length_search)


def placement_list(cfg):
    """(dz, dy, dx) per placement in the reference's loop order (:270-279): dz outer, dy, dx inner."""
    return [(float(dz), float(dy), float(dx)) for dz in cfg.height_search for dy in cfg.width_search
            for dx in cfg.length_search]


def gripper_bound(cfg):
    """GRIPPER_BOUND (configs/config.py:58-64) as (8, 3) fp32 values."""
    return np.array([[x, y, z] for x in (cfg.finger_length, -cfg.bottom_length)
                     for y in (cfg.half_bottom_width, -cfg.half_bottom_width)
                     for z in (cfg.half_hand_thickness, -cfg.half_hand_thickness)], np.float32)


def rigid_inverse(g2l, dtype=np.float64):
    """[R^T | -R^T t] of (F, 4, 4) transforms, in `dtype` (fp32: the products and sums in the kernel's order)."""
    g = np.asarray(g2l, np.float32).astype(dtype)
    out = np.zeros(g.shape, dtype)
    Rt = np.swapaxes(g[:, :3, :3], 1, 2)
    out[:, :3, :3] = Rt
    t = g[:, :3, 3]
    for i in range(3):
        out[:, i, 3] = -((Rt[:, i, 0] * t[:, 0] + Rt[:, i, 1] * t[:, 1]) + Rt[:, i, 2] * t[:, 2])
    out[:, 3, 3] = 1
    return out


def _regions(lx, ly, lz, cfg, dz, dy, dx, dt, tol, sabotage):
    """finger, close, behind masks of one placement; tol > 0 widens every interval, tol < 0 narrows it."""
    f = lambda v: dt(np.float32(v))                                              # noqa: E731  (rounded to fp32 once)
    hht, hbs, hbw = cfg.half_hand_thickness, cfg.half_bottom_space, cfg.half_bottom_width
    tol = dt(tol)
    z_bool = (lz < f(hht + dz) + tol) & (lz > f(-hht + dz) - tol)
    sdy = -dy if "flip_dy" in sabotage else dy
    y_bool = (ly < f(hbs + sdy) + tol) & (ly > f(-hbs + sdy) - tol)
    abs_y = np.abs(ly if "abs_no_dy" in sabotage else ly + f(dy))
    y_coll = (abs_y > f(hbs) - tol) & (abs_y < f(hbw) + tol)
    x_bool = (lx > f(-cfg.bottom_length + dx) - tol) & (lx < f(cfg.finger_length + dx) + tol)
    close = x_bool & z_bool & y_bool
    return z_bool & x_bool & y_coll, close, close & (lx < f(cfg.back_collision_margin) + tol)


def grade(g2l, xyz, labels, cfg=None, frame_count=None, dtype=np.float64, sabotage=()):
    """g2l (F, 4, 4), xyz (3, M) fp32, labels (M,) -> dict of `ints` (F, P, 4) = {finger, close, behind, multi_label},
    `table`, `valid`, `label`, `fail` (F,) as include/s4g_ops.h defines them for s4g_contact_search_f32, `near` (F,)
    bool (a region boundary or the table plane within TOL: what `decided` reads) and `raises` (F,) bool: the
    reference would raise on this frame (it reaches an empty close region before a failing test, :283-286)."""
    cfg = cfg or Config()
    dt = np.dtype(dtype).type
    G = np.asarray(g2l, np.float32)
    F = G.shape[0]
    p = np.asarray(xyz, np.float32).astype(dtype)
    lab = np.asarray(labels)
    pl = placement_list(cfg)
    P = len(pl)
    rows = F if frame_count is None or "ignore_frame_count" in sabotage else max(0, min(F, int(frame_count)))
    out = {"ints": np.zeros((F, P, 4), np.int32), "table": np.zeros(F, np.int32), "valid": np.zeros(F, np.int32),
           "label": np.full(F, cfg.no_label, np.int32), "fail": np.zeros(F, np.int32), "near": np.zeros(F, bool),
           "raises": np.zeros(F, bool)}
    l2g = rigid_inverse(G, dtype)
    corners = gripper_bound(cfg).astype(dtype)
    limit = dt(np.float32(cfg.table_height + cfg.table_collision_offset))
    fin = np.isfinite(p).all(0)
    for f in range(rows):
        if not np.isfinite(G[f]).all():
            out["fail"][f] = FAIL_NONFINITE
            continue
        g = G[f].astype(dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            loc = [((g[r, 0] * p[0] + g[r, 1] * p[1]) + g[r, 2] * p[2]) + g[r, 3] for r in range(3)]
        shifts = [(0.0, 0.0, 0.0)] if "real_table" not in sabotage else [(dx, dy, dz) for dz, dy, dx in pl]
        bits, near = 0, False
        for sx, sy, sz in shifts:
            c = corners + np.array([sx, sy, sz], dtype)
            z = ((l2g[f, 2, 0] * c[:, 0] + l2g[f, 2, 1] * c[:, 1]) + l2g[f, 2, 2] * c[:, 2]) + l2g[f, 2, 3]
            if (z < limit).any():
                bits |= FAIL_TABLE
            near = near or bool((np.abs(z - limit) < TOL).any())
        out["table"][f] = bits & 1
        first_fail = None
        for k, (dz, dy, dx) in enumerate(pl):
            with np.errstate(invalid="ignore"):
                fing, close, behind = (m & fin for m in _regions(*loc, cfg, dz, dy, dx, dt, 0.0, sabotage))
                if dtype == np.float64:
                    wide = _regions(*loc, cfg, dz, dy, dx, dt, TOL, sabotage)
                    narrow = _regions(*loc, cfg, dz, dy, dx, dt, -TOL, sabotage)
                    near = near or any(bool(((w ^ n) & fin).any()) for w, n in zip(wide, narrow))
            nf, nc = int(fing.sum()), int(close.sum())
            nb = 0 if "no_behind" in sabotage else int(behind.sum())
            multi = int(nc > 0 and len(np.unique(lab[close])) > 1)
            out["ints"][f, k] = (nf, nc, int(behind.sum()), multi)
            here = (FAIL_FINGER if nf else 0) | (FAIL_EMPTY if nc == 0 else 0) | (FAIL_BEHIND if nb else 0) | \
                   (FAIL_LABELS if multi else 0)
            if first_fail is None and here and not (bits & FAIL_TABLE):
                first_fail = here
                out["raises"][f] = nf == 0 and nc == 0            # min() of an empty tensor (:286)
            bits |= here
        out["fail"][f], out["near"][f] = bits, near
        if bits == 0:
            out["valid"][f] = 1
            k = 0 if "first_label" in sabotage else P - 1
            close = _regions(*loc, cfg, *pl[k], dt, 0.0, sabotage)[1] & fin
            out["label"][f] = lab[close].min()
    return out


def nearest(query, scene, radius):
    """The `max_nn = 1` hybrid search (:143-145) as a float64 brute force: query (3, N), scene (3, M) fp32 -> (`nearest`
    (N,) int32, -1 without a scene point with d^2 < r^2 or where the query is not finite; the lower index wins a tie),
    `near` (N,) bool: what `decided` reads)."""
    q = np.asarray(query, np.float32).astype(np.float64).T
    p = np.asarray(scene, np.float32).astype(np.float64).T
    r2 = float(radius) ** 2
    idx, near = np.full(len(q), -1, np.int32), np.zeros(len(q), bool)
    for i in range(len(q)):
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = ((p - q[i]) ** 2).sum(1)
            inside = np.nonzero(d2 < r2)[0]
            near[i] = bool((np.abs(d2 - r2) < ULP4 * r2).any())
        if len(inside):
            o = inside[np.lexsort((inside, d2[inside]))]
            idx[i] = o[0]
            if len(o) > 1 and d2[o[1]] - d2[o[0]] < ULP4 * d2[o[1]]:
                near[i] = True
    return idx, near


def frame_scores(search, antipodal, dtype=np.float64, sabotage=()):
    """min(log(search) / 6.5, 1) * antipodal (:189-193); a NaN stays, as torch.min keeps it."""
    dt = np.dtype(dtype).type
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.log(np.asarray(search, np.float32).astype(dtype)) / dt(6.5)
        if "no_min" not in sabotage:
            s = np.where(np.isnan(s), s, np.minimum(s, dt(1.0)))
        return (s * np.asarray(antipodal, np.float32).astype(dtype)).astype(dtype)


def select(nearest_idx, cloud, scene_normals, camera, frame_point_index, valid, search, antipodal, frame_count=None,
           dtype=np.float64, sabotage=()):
    """The rest of `_find_match` and of `run_score` per view point -> dict of `normals` (N, 3) float64, `best_frame`,
    `point_score`, `valid_index` (N,) padded with -1, `count`, `tie` (N,) bool (what `decided` reads)."""
    q = np.asarray(cloud, np.float32).astype(np.float64).T
    nrm = np.asarray(scene_normals, np.float32).astype(np.float64).T
    cam = np.asarray(camera, np.float32).astype(np.float64)
    fpi = np.asarray(frame_point_index).astype(np.int64)
    F, N = len(fpi), len(q)
    rows = F if frame_count is None or "ignore_frame_count" in sabotage else max(0, min(F, int(frame_count)))
    sc = frame_scores(search, antipodal, dtype, sabotage)
    s32, a32 = np.asarray(search, np.float32), np.asarray(antipodal, np.float32)
    out = {"normals": np.zeros((N, 3)), "best_frame": np.full(N, -1, np.int32), "point_score": np.zeros(N, dtype),
           "valid_index": np.full(N, -1, np.int32), "count": 0, "tie": np.zeros(N, bool)}
    for j in range(N):
        i = int(nearest_idx[j])
        n = np.array([0.0, 0.0, 1.0])
        if i >= 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                n = nrm[i] / np.sqrt((nrm[i] * nrm[i]).sum())                    # :166
        with np.errstate(invalid="ignore", over="ignore"):
            ref = cam - q[j]
        if np.isfinite(ref).all():                                               # orient_normals_towards_camera_location
            if not np.isnan(n).any() and not n.any():
                rl = float(np.sqrt((ref * ref).sum()))
                n = ref / rl if rl > 0.0 else np.array([0.0, 0.0, 1.0])
            elif float(n[0] * ref[0] + n[1] * ref[1] + n[2] * ref[2]) < 0.0:
                n = -n
        out["normals"][j] = n
        if i < 0:
            continue
        best, arg = np.dtype(dtype).type(0.0), -1
        mine = [f for f in np.nonzero(fpi[:rows] == i)[0] if valid[f]]           # ascending frame index (:152, :198)
        for f in mine:                                                           # :200-206
            if best >= sc[f] if "earlier_wins" in sabotage else best > sc[f]:
                continue
            best, arg = sc[f], f
        out["point_score"][j] = best
        if best > 0:
            out["best_frame"][j] = arg
        if len(mine) > 1:
            o = sorted(mine, key=lambda f: -sc[f] if sc[f] == sc[f] else np.inf)
            a, b = o[0], o[1]
            same = s32[a] == s32[b] and a32[a] == a32[b]
            out["tie"][j] = bool(np.isnan(sc[[a, b]]).any() or
                                 (not same and abs(sc[a] - sc[b]) < 1e-6 * max(abs(sc[a]), abs(sc[b]))))
    vi = np.nonzero(out["best_frame"] >= 0)[0]
    out["valid_index"][:len(vi)] = vi
    out["count"] = len(vi)
    return out


def label(reference_cloud, cloud, scene, scene_normals, labels, camera, g2l, frame_point_index, search, antipodal,
          radius, cfg=None, frame_count=None, dtype=np.float64, sabotage=()):
    """All three layers on one scene -> (grade dict, (nearest, near), select dict).  sabotage "match_noisy" runs the
    match on the noisy cloud, "orient_reference" orients against the reference point."""
    g = grade(g2l, scene, labels, cfg, frame_count, dtype, sabotage)
    nn = nearest(cloud if "match_noisy" in sabotage else reference_cloud, scene, radius)
    s = select(nn[0], reference_cloud if "orient_reference" in sabotage else cloud, scene_normals, camera,
               frame_point_index, g["valid"], search, antipodal, frame_count, dtype, sabotage)
    return g, nn, s


def decided(g, nn, s, frame_point_index):
    """-> (frames (F,) bool, view points (N,) bool): the rows an fp32 implementation is held to.  A view point is
    undecided too where a frame of its scene point is."""
    kf = ~g["near"]
    fpi = np.asarray(frame_point_index)
    bad_points = set(fpi[~kf].tolist())
    kp = ~nn[1] & ~s["tie"] & np.array([int(i) not in bad_points for i in nn[0]])
    return kf, kp


SABOTAGES = ("flip_dy", "abs_no_dy", "no_behind", "first_label", "earlier_wins", "match_noisy", "orient_reference",
             "no_min", "real_table", "ignore_frame_count")


def altered_rows(fx, name, base=None):
    """How many kept rows of the fixture `fx` (the arrays of tests/golden/contact_search.npz) the mistake `name`
    changes: frames whose integers, verdicts, failure bits or label differ, plus view points whose nearest index,
    normal, best frame or score differ."""
    args = (fx["reference_cloud"], fx["cloud"], fx["scene"], fx["scene_normals"], fx["labels"], fx["camera"],
            fx["g2l"], fx["frame_point_index"], fx["search_score"], fx["antipodal_score"], float(fx["radius"][0]))
    fc = int(fx["frame_count"][0])
    g0, n0, s0 = base or label(*args, frame_count=fc)
    g1, n1, s1 = label(*args, frame_count=fc, sabotage=(name,))
    kf, kp = fx["keep_frames"].astype(bool), fx["keep_points"].astype(bool)
    df = (g0["ints"] != g1["ints"]).any((1, 2)) | (g0["valid"] != g1["valid"]) | (g0["label"] != g1["label"]) | \
         (g0["fail"] != g1["fail"]) | (g0["table"] != g1["table"])
    with np.errstate(invalid="ignore"):
        dp = (n0[0] != n1[0]) | (np.abs(s0["normals"] - s1["normals"]).max(1) > 1e-6) | \
             (s0["best_frame"] != s1["best_frame"]) | (np.abs(s0["point_score"] - s1["point_score"]) > 1e-6)
    return int((df & kf).sum()) + int((dp & kp).sum())
