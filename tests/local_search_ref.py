"""Float64 yardstick of the data generator's local grasp search (`postprocess.grade_local_search`,
csrc/local_search.hip; the reference's `TorchSingleViewPointCloud.finger_hand`, `_table_collision_check` and
`_antipodal_score`, data_gen/pcd_classes/torch_single_view_point_cloud.py:152-180,224-358).  TEST INFRASTRUCTURE ONLY.

  * `search64`    every output of the call in float64 (exact products of the fp32 inputs and of the fp32 cos / sin the
                  reference forms), one frame at a time on freshly zeroed results (decision "no stale slots"), plus
                  per frame whether it is DECIDED at `tol`.
  * `decided`     the frames whose every verdict no point closer than `tol` to a boundary can turn: the two frame
                  gates, no table corner within `tol` of the table plane, slab counts whose threshold lies outside
                  [n - ambiguous, n + ambiguous], and per placement the gates in the reference's order -- the first
                  one that certainly skips decides the placement; one that reaches the score needs an exact close
                  count (no ambiguous close-region point), one certain label, no point within `tol` of a band bound and
                  a score away from the 1e-4 validity line.
  * `face_scene`  an identity frame at the origin, roll 0 only (cos 1, sin 0: every transform exact in fp32): points
                  exactly on, one ulp inside and one ulp outside every region face, slab bound and band bound.

The kernels' loop structure (what the edge shapes of tests/test_local_search_gpu.py cross): point chunks per scene =
ceil(N / 16 384) within [4, 64] (empty below N = 4); sweeps of 1 024 points; 32 workgroups share a scene's frames, 8
frames per workgroup and pass, so a pass holds 256 frames."""
import numpy as np

SCORE_TOL = 1e-4            # the bar of tests/test_eval_frames_gpu.py for this same score (its scale is 1)
FRAMES_PER_PASS = 256       # csrc/local_search.hip: LS_GX * LS_SLOTS
CHUNK_POINTS = 16384        # LS_CHUNK_POINTS (4 chunks at least: the count turns at N = 65 536 / 65 537)
REASONS = ("scored", "table", "slab", "back", "finger", "few", "labels", "frame")


def _f32(v):
    return float(np.float32(v))


def constants(cfg):
    """The fp32 values the kernels and the reference compare against, as float64."""
    tb = cfg.tables()
    c = {k: tb[k].numpy().astype(np.float64) for k in tb}
    c.update(fl=_f32(cfg.finger_length), bl=_f32(cfg.bottom_length), hht=_f32(cfg.half_hand_thickness),
             hbw=_f32(cfg.half_bottom_width), hbs=_f32(cfg.half_bottom_space), m=_f32(cfg.back_collision_margin),
             back_thr=_f32(cfg.back_collision_threshold), fing_thr=_f32(cfg.finger_collision_threshold),
             min_points=_f32(cfg.close_region_min_points), nd=_f32(cfg.neighbor_depth), th=_f32(cfg.table_height),
             tl=_f32(cfg.table_height + cfg.table_collision_offset), slab_thr=_f32(cfg.num_points_threshold))
    return c


def _near(v, faces, tol):
    out = np.zeros(v.shape, bool)
    for f in faces:
        out |= np.abs(v - f) < tol
    return out


def search64(points, frames, cloud, normals, labels, cfg, tol=4e-6, frame_count=None, band_f32=False, clear_tol=None):
    """points (F, 3), frames (F, 3, 3), cloud / normals (3, N) fp32, labels (N,) -> dict of numpy arrays: (F, L, T)
    `search_score`, `objects_label`, `back`, `finger`, `close` (int64), `table_collision` (bool), `antipodal_score`
    (float64), `reason` (index into REASONS: why the placement was skipped, 0 = scored), `clear` (no point within tol
    (or `clear_tol`, where given) of a face of the placement's three regions: any fp32 route counts the same integers); (F, L) `slab_count` and `amb_slab` (points within tol of a
    slab bound: an fp32 count may differ by that many); (F,)
    `valid`, `gate` (the frame passed both gates), `decided`; `valid_index` (F,) ascending, -1 padded; `count`.
    band_f32: the band bounds in fp32 arithmetic on the extrema -- for scenes whose local coordinates are exact fp32
    values (`face_scene`), where it makes every integer the exact fp32 answer."""
    k = constants(cfg)
    L, T = cfg.shape
    F = len(points)
    n_live = F if frame_count is None else max(0, min(F, int(frame_count)))
    P = np.asarray(cloud, np.float64)
    Nn = np.asarray(normals, np.float64)
    lab = np.asarray(labels).astype(np.int64)
    out = {n: np.zeros((F, L, T), np.int64) for n in ("search_score", "back", "finger", "close")}
    out["objects_label"] = np.full((F, L, T), cfg.no_label, np.int64)
    out["table_collision"] = np.zeros((F, L, T), bool)
    out["antipodal_score"] = np.zeros((F, L, T), np.float64)
    out["reason"] = np.full((F, L, T), 7, np.int64)
    out["clear"] = np.zeros((F, L, T), bool)
    out["slab_count"] = np.zeros((F, L), np.int64)
    out["amb_slab"] = np.zeros((F, L), np.int64)
    out["valid"] = np.zeros(F, bool)
    out["gate"] = np.zeros(F, bool)
    out["decided"] = np.ones(F, bool)
    corners = np.array([[x, y, z] for x in (k["fl"], -k["bl"]) for y in (k["hbw"], -k["hbw"]) for z in (k["hht"], -k["hht"])])
    r2lim = (k["hbw"] ** 2 + k["hht"] ** 2) * 1.01 + 1e-6
    for f in range(n_live):
        R = np.asarray(frames[f], np.float64)
        p = np.asarray(points[f], np.float64)
        mean = np.abs(R).mean()
        reach = p[2] + R[2, 0] * k["fl"]
        if not (np.isfinite(R).all() and np.isfinite(p).all()):
            out["decided"][f] = False
            continue
        if abs(mean - 1e-6) < 1e-8 or abs(reach - k["th"]) < tol:
            out["decided"][f] = False
        if mean < 1e-6 or reach < k["th"]:                                   # :257,259
            continue
        out["gate"][f] = True
        decided = True
        # the table gate (:224-241): row 2 of [R | p] @ LOCAL_SEARCH_TO_LOCAL
        table = np.zeros((L, T), bool)
        for d in range(L):
            for t in range(T):
                c, s = k["cos"][t], k["sin"][t]
                m = np.array([R[2, 0], R[2, 1] * c + R[2, 2] * s, -R[2, 1] * s + R[2, 2] * c])
                zc = corners @ m + (R[2, 0] * k["depth"][d] + p[2])
                table[d, t] = (zc < k["tl"]).any()
                decided &= not (np.abs(zc - k["tl"]) < tol).any()
        out["table_collision"][f] = table
        loc = R.T @ P + (-(R.T @ p))[:, None]                                # :91-94, :265
        x, y, z = loc
        nl = R.T @ Nn                                                        # :267
        near_lo = np.stack([np.abs(x - k["lo"][d]) < tol for d in range(L)])
        near_hi = np.stack([np.abs(x - k["hi"][d]) < tol for d in range(L)])
        slab = np.stack([(x < k["hi"][d]) & (x > k["lo"][d]) for d in range(L)])          # :270-271
        n_slab = slab.sum(1)
        a_slab = (near_lo | near_hi).sum(1)
        out["slab_count"][f] = n_slab
        slab_skip = n_slab < k["slab_thr"]                                                # :273
        decided &= bool(((n_slab - a_slab >= k["slab_thr"]) | (n_slab + a_slab < k["slab_thr"])).all())
        out["amb_slab"][f] = a_slab
        keep = ((slab | near_lo | near_hi).any(0)) & (y * y + z * z < r2lim)
        x, y, z, ny, nz, lb = x[keep], y[keep], z[keep], nl[1][keep], nl[2][keep], lab[keep]
        slab, near_x = slab[:, keep], (near_lo | near_hi)[:, keep]
        for t in range(T):
            c, s = k["cos"][t], k["sin"][t]
            yy, zz = c * y + s * z, -s * y + c * z                           # config.py:79-82
            an = np.abs(c * ny + s * nz)                                     # :339-341, :173-174
            zin = (zz < k["hht"]) & (zz > -k["hht"])
            wide_yz = (np.abs(zz) < k["hht"] + tol) & (np.abs(yy) < k["hbw"] + tol)
            near_z = _near(zz, (k["hht"], -k["hht"]), tol)
            for d in range(L):
                xs = x - k["depth"][d]
                sl = slab[d]
                back = sl & zin & (yy < k["hbw"]) & (yy > -k["hbw"]) & (xs < -k["m"])     # :297-300
                fing = sl & zin & (((yy < k["hbw"]) & (yy > k["hbs"])) | ((yy > -k["hbw"]) & (yy < -k["hbs"])))
                closer = sl & zin & (yy < k["hbs"]) & (yy > -k["hbs"])                    # :317-319
                wide = (sl | near_x[d]) & wide_yz
                edge = near_x[d] | near_z
                a_back = (wide & (xs < -k["m"] + tol) & (edge | _near(yy, (k["hbw"], -k["hbw"]), tol)
                                                         | (np.abs(xs + k["m"]) < tol))).sum()
                a_fing = (wide & (edge | _near(yy, (k["hbw"], -k["hbw"], k["hbs"], -k["hbs"]), tol))).sum()
                amb_c = wide & (np.abs(yy) < k["hbs"] + tol) & (edge | _near(yy, (k["hbs"], -k["hbs"]), tol))
                nb, nf, ncl = int(back.sum()), int(fing.sum()), int(closer.sum())
                if clear_tol is None:
                    out["clear"][f, d, t] = a_back + a_fing + int(amb_c.sum()) == 0
                else:                                                        # the same faces at a tolerance of its own
                    w2 = (sl | (_near(x, (k["lo"][d], k["hi"][d]), clear_tol))) & (np.abs(zz) < k["hht"] + clear_tol) \
                        & (np.abs(yy) < k["hbw"] + clear_tol)
                    out["clear"][f, d, t] = not (w2 & (_near(x, (k["lo"][d], k["hi"][d]), clear_tol)
                                                       | _near(zz, (k["hht"], -k["hht"]), clear_tol)
                                                       | _near(yy, (k["hbw"], -k["hbw"], k["hbs"], -k["hbs"]), clear_tol)
                                                       | (np.abs(xs + k["m"]) < clear_tol))).any()
                if not table[d, t]:                                          # (skipped before anything is counted, :288)
                    out["back"][f, d, t], out["finger"][f, d, t], out["close"][f, d, t] = nb, nf, ncl
                side = lambda n, a, thr: (n - a > thr) or (n + a <= thr)
                if table[d, t]:
                    out["reason"][f, d, t] = 1
                    continue
                if slab_skip[d]:
                    out["reason"][f, d, t] = 2
                    continue
                decided &= side(nb, a_back, k["back_thr"])
                if nb > k["back_thr"]:                                       # :302
                    out["reason"][f, d, t] = 3
                    continue
                decided &= side(nf, a_fing, k["fing_thr"])
                if nf > k["fing_thr"]:                                       # :313
                    out["reason"][f, d, t] = 4
                    continue
                a_close = int(amb_c.sum())
                decided &= (ncl - a_close >= k["min_points"]) or (ncl + a_close < k["min_points"])
                if ncl < k["min_points"] or ncl == 0:                        # :323
                    out["reason"][f, d, t] = 5
                    continue
                sure = closer & ~amb_c
                ls = lb[sure]
                two_sure = ls.size > 0 and ls.min() != ls.max()
                lc = lb[closer]
                if lc.min() != lc.max():                                     # :326-330
                    out["reason"][f, d, t] = 6
                    decided &= bool(two_sure)
                    continue
                decided &= a_close == 0                                      # the search score is the exact count
                out["reason"][f, d, t] = 0
                out["search_score"][f, d, t] = ncl
                out["objects_label"][f, d, t] = lc[0]
                cy, ca = yy[closer], an[closer]
                left_y, right_y = cy.max(), cy.min()                         # :167-168
                if band_f32:
                    l32, r32 = np.float32(left_y), np.float32(right_y)
                    dep = min((l32 - r32) / np.float32(3), np.float32(k["nd"]))
                    lthr, rthr = float(l32 - dep), float(r32 + dep)
                else:
                    dep = min((left_y - right_y) / 3, k["nd"])               # :169
                    lthr, rthr = left_y - dep, right_y + dep
                il, ir = cy > lthr, cy < rthr                                # :171-172
                decided &= not (_near(cy, (lthr, rthr), tol).any())
                with np.errstate(invalid="ignore", divide="ignore"):
                    sc = (ca[il].sum() / il.sum()) * (ca[ir].sum() / ir.sum()) if True else 0.0   # :176
                out["antipodal_score"][f, d, t] = sc
                if np.isnan(sc) or abs(sc - 1e-4) < 2e-5:
                    decided = False
        sc = out["antipodal_score"][f]
        out["valid"][f] = not (np.nanmax(sc) < 1e-4) if not np.isnan(sc).any() else True    # :348
        out["decided"][f] &= bool(decided)
    vi = np.nonzero(out["valid"])[0]
    out["valid_index"] = np.concatenate([vi, np.full(F - len(vi), -1, np.int64)])
    out["count"] = len(vi)
    return out


def decided(r):
    """Boolean per frame: see the module docstring."""
    return r["decided"]


def frames_of(points, frames, cfg):
    """`valid_frame` (:351-356) in float64: (F, L, T, 4, 4) = [R | p] @ LOCAL_SEARCH_TO_LOCAL."""
    S = cfg.search_to_local().numpy().astype(np.float64)
    F = len(points)
    H = np.zeros((F, 4, 4))
    H[:, :3, :3], H[:, :3, 3], H[:, 3, 3] = frames, points, 1
    return np.einsum("fij,ltjk->fltik", H, S)


def composed_poses(points, frames, cfg):
    """The L * T poses per frame whose `eval_frames` grading (inverse="se3") is the route the parent commit already
    offers: fp32 (F, L * T, 4, 4)."""
    L, T = cfg.shape
    return frames_of(points, frames, cfg).reshape(len(points), L * T, 4, 4).astype(np.float32)


def face_config(**kw):
    """The configuration of `face_scene`: roll 0 only (cos = 1, sin = 0 exactly), two depths that are exact fp32
    values, a table far below, NEIGHBOR_DEPTH = 2^-8, 4 points make a close region."""
    from s4g_release_amd.postprocess import LocalSearchConfig
    base = dict(theta_search_deg=(0,), length_search=(-0.0625, -0.03125), table_height=-1.0, neighbor_depth=2.0 ** -8,
                close_region_min_points=4, back_collision_threshold=1e4, finger_collision_threshold=1e4,
                num_points_threshold=1)
    base.update(kw)
    return LocalSearchConfig(**base)


def face_scene(cfg):
    """-> (points (1, 3), frames (1, 3, 3), cloud (3, M), normals (3, M) fp32, labels (M,) int32).  Local coordinates
    ARE the cloud's (identity frame at the origin, roll 0); x - dl is exact next to a face (Sterbenz).  Points exactly
    on, one ulp inside and one ulp outside: both bounds of both depth slabs; x = dl - margin (behind the palm) for
    both depths; z = +-half_hand_thickness; y = +-half_bottom_width and +-half_bottom_space; and both band bounds
    +-(Y - 2^-8), Y = one ulp inside half_bottom_space being the close region's extremum.  The points on the band
    bounds carry |n.y| = 1 and all others 0.125, so one wrong band membership moves the score by far more than 1e-4."""
    k = constants(cfg)
    f32 = np.float32
    up = lambda v: float(np.nextafter(f32(v), f32(np.inf)))
    dn = lambda v: float(np.nextafter(f32(v), f32(-np.inf)))
    three = lambda v: (float(f32(v)), up(v), dn(v))
    xin = float(f32(-0.015625))                       # inside both slabs, in front of both palms
    Y = dn(k["hbs"])
    bound = Y - 2.0 ** -8
    assert k["nd"] == 2.0 ** -8 and 2 * Y / 3 > 2.0 ** -8 and float(f32(bound)) == bound
    pts, nrm = [], []
    for d in range(len(k["depth"])):
        for v in (k["lo"][d], k["hi"][d], k["depth"][d] - k["m"]):
            pts += [(w, 0.0, 0.0) for w in three(v)]
    for v in (k["hht"], -k["hht"]):
        pts += [(xin, 0.001, w) for w in three(v)]
    for v in (k["hbw"], -k["hbw"], k["hbs"], -k["hbs"]):
        pts += [(xin, w, 0.0) for w in three(v)]
    nrm += [(0.0, 0.125, 0.0)] * len(pts)
    pts += [(xin, Y, 0.0), (xin, -Y, 0.0), (xin, 0.0, 0.0)]
    nrm += [(0.0, 0.125, 0.0)] * 3
    for v in (bound, -bound):
        pts += [(xin, w, 0.0) for w in three(v)]
        nrm += [(0.0, 1.0, 0.0)] * 3
    cloud = np.array(pts, np.float32).T.copy()
    normals = np.array(nrm, np.float32).T.copy()
    labels = np.full(cloud.shape[1], 3, np.int32)
    return np.zeros((1, 3), np.float32), np.eye(3, dtype=np.float32)[None].copy(), cloud, normals, labels


def noisy_normals(rng, n):
    v = rng.standard_normal((3, n))
    v /= np.linalg.norm(v, axis=0, keepdims=True)
    return (v * (1 + rng.uniform(-0.02, 0.02, n))).astype(np.float32)


def box_scene(rng, n_points, n_frames, cfg, n_boxes=3):
    """A small table-top scene for the loop-edge tests: a table at TABLE_HEIGHT and `n_boxes` boxes on it (the last two
    a close pair), n_points points in all with noisy unit normals and labels (table 0, boxes 1..), and n_frames side /
    top grasp frames on box faces with a small jitter.  -> (points (F, 3), frames (F, 3, 3), cloud (3, N), normals
    (3, N) fp32, labels (N,) int32)."""
    th = cfg.table_height
    centres = [(-0.15, -0.1), (0.1, 0.12), (0.134, 0.12), (-0.05, 0.2), (0.2, -0.15)][:n_boxes]
    sizes = [(0.04, 0.05, 0.10), (0.03, 0.04, 0.08), (0.03, 0.04, 0.08), (0.05, 0.03, 0.03), (0.04, 0.04, 0.1)][:n_boxes]
    n_table = n_points // 4
    per = [(n_points - n_table) // n_boxes] * n_boxes
    per[0] += n_points - n_table - sum(per)
    pts = [np.stack([rng.uniform(-0.3, 0.3, n_table), rng.uniform(-0.3, 0.3, n_table), np.full(n_table, th)], 1)]
    nrm = [np.tile([0, 0, 1.0], (n_table, 1))]
    lab = [np.zeros(n_table, int)]
    for i, ((cx, cy), size, n) in enumerate(zip(centres, sizes, per)):
        areas = np.array([size[1] * size[2]] * 2 + [size[0] * size[2]] * 2 + [size[0] * size[1]])
        face = rng.choice(5, size=n, p=areas / areas.sum())
        q, nn = np.zeros((n, 3)), np.zeros((n, 3))
        u, v = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
        for fi, (axis, sign) in enumerate(((0, 1), (0, -1), (1, 1), (1, -1), (2, 1))):
            m = face == fi
            a, b = [j for j in range(3) if j != axis]
            q[m, axis] = sign * 0.5 * size[axis]
            q[m, a], q[m, b] = u[m] * size[a], v[m] * size[b]
            nn[m, axis] = sign
        q[:, 2] += 0.5 * size[2] + th
        q[:, 0] += cx
        q[:, 1] += cy
        pts.append(q); nrm.append(nn); lab.append(np.full(n, i + 1))
    pts, nrm, lab = np.concatenate(pts), np.concatenate(nrm), np.concatenate(lab)
    nrm = nrm + rng.normal(0, 0.05, nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o = rng.permutation(len(pts))
    P, Fr = np.zeros((n_frames, 3)), np.zeros((n_frames, 3, 3))
    for f in range(n_frames):
        i = int(rng.integers(n_boxes))
        (cx, cy), size = centres[i], sizes[i]
        if rng.random() < 0.3:                                              # from above: x = down
            x = np.array([0.0, 0.0, -1.0])
            yaw = rng.uniform(-0.3, 0.3)
            y = np.array([np.cos(yaw), np.sin(yaw), 0.0])
            origin = np.array([cx + rng.uniform(-0.005, 0.005), cy + rng.uniform(-0.005, 0.005), th + size[2]])
        else:                                                               # from a side: x = horizontal, into a y face
            sgn = rng.choice([-1.0, 1.0])
            yaw = rng.uniform(-0.2, 0.2)
            x = np.array([np.sin(yaw), -sgn * np.cos(yaw), 0.0])
            y = np.array([0.0, 0.0, 1.0]) if rng.random() < 0.5 else np.cross(np.array([0.0, 0.0, 1.0]), x)
            origin = np.array([cx + rng.uniform(-0.005, 0.005), cy + sgn * 0.5 * size[1],
                               th + size[2] * rng.uniform(0.3, 0.9)])
        y = y - x * (x @ y)
        y /= np.linalg.norm(y)
        Fr[f] = np.stack([x, y, np.cross(x, y)], 1)
        P[f] = origin
    return (P.astype(np.float32), Fr.astype(np.float32), pts[o].T.astype(np.float32).copy(),
            nrm[o].T.astype(np.float32).copy(), lab[o].astype(np.int32))


def blob_scene(rng, n_points, n_frames, cfg):
    """A small decided scene for the loop-edge tests, built in the local frame of a base grasp 30 cm above the table
    (both frame gates pass and no corner comes near the table plane, whatever the roll).  Of the first 96 points, four
    fifths lie in a blob between the fingers of the base frame's placement (last depth, roll 0) -- x in (-15 mm, 60 mm),
    |y| < 30 mm, |z| < 10 mm, label 1 -- and the rest are clutter in a 30 cm cube around it with label 2, which fills
    fingers and palms of some placements.  Every further point lies on the table top, 30 cm below (label 0): outside
    every gripper box, but inside depth slabs, so the slab counters run over the whole cloud.  (More points near the
    gripper would leave no frame decided: with 48 placements per frame, some point sits within the tolerance of a face.)  The frames are the base frame turned by up to 0.2 rad about a random axis and moved by up to
    5 mm: every frame sees the blob, so from about a hundred points on placements are scored, skipped for collisions
    and skipped for two labels in every frame.  -> (points (F, 3), frames (F, 3, 3), cloud (3, N), normals (3, N)
    fp32, labels (N,) int32)."""
    def rot(axis, ang):
        axis = axis / np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    base = rot(rng.standard_normal(3), rng.uniform(0, np.pi))
    origin = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), cfg.table_height + 0.3])
    n_near = min(n_points, 96)
    n_blob = n_near - n_near // 5
    loc = np.stack([rng.uniform(-0.015, 0.06, n_blob), rng.uniform(-0.03, 0.03, n_blob), rng.uniform(-0.01, 0.01, n_blob)], 1)
    clutter = rng.uniform(-0.15, 0.15, (n_near - n_blob, 3))
    n_far = n_points - n_near
    far = np.stack([rng.uniform(-0.3, 0.3, n_far), rng.uniform(-0.3, 0.3, n_far), np.full(n_far, cfg.table_height)], 1)
    pts = np.concatenate([np.concatenate([loc, clutter]) @ base.T + origin, far])
    lab = np.concatenate([np.ones(n_blob, int), np.full(n_near - n_blob, 2), np.zeros(n_far, int)])
    o = rng.permutation(n_points)
    P, Fr = np.zeros((n_frames, 3)), np.zeros((n_frames, 3, 3))
    for f in range(n_frames):
        Fr[f] = rot(rng.standard_normal(3), rng.uniform(0, 0.2)) @ base if f else base
        P[f] = origin + (rng.uniform(-0.005, 0.005, 3) if f else 0)
    return (P.astype(np.float32), Fr.astype(np.float32), pts[o].T.astype(np.float32).copy(),
            noisy_normals(rng, n_points), lab[o].astype(np.int32))
