"""Float64 yardstick of the curvature model's per-object data (`postprocess.estimate_object_frames`,
`grade_object_frames`; csrc/darboux.hip, csrc/darboux_object.hip; the reference's `GenerateDarbouxObjectData`,
data_gen/data_generator/data_object_darboux_generator.py:62-247).  TEST INFRASTRUCTURE ONLY.

  * `frames64`  `_estimate_frame` (:62-92) in numpy on one object with a brute-force radius search (`d^2 < r^2`, the
                point itself included): the normalised mean normal, the SCALAR `M = I - (n.n)` as written, the
                eigenvector of the smallest eigenvalue, [-n, -principal, minor] and [n, principal, minor]; plus what
                says how well a frame is determined (tests/darboux_ref.py: `near`, `gap`, `minor_norm`).
  * `grade64`   `finger_hand_view` with `_antipodal_score` (:131-247) per (frame, direction): local coordinates in
                float64 from the fp32 frames (exact products), counts per (depth, roll, shift), the fold over the shifts
                in the reference's order with its fp32 `temp += n / 3`, the truncated search score, the antipodal score
                in float64 -- and per placement whether it is DECIDED at `eps`.
  * the decided rule (crude on purpose): a placement is undecided when a point of its wide box (every region widened
                by eps) lies within eps of a bound of any region -- slab, palm plane, +-HBW, +-HBS, the z window of any
                shift --, when the slab count could cross NUM_POINTS_THRESHOLD by the points within eps of a slab
                bound, when a close-region point lies within eps of a band bound, or when the score is NaN.
  * `SABOTAGES` variants of `grade64` that each get one thing wrong; tests/test_darboux_object_ref.py shows that every
                one of them changes kept rows of the fixture.

The kernels' loop structure (what the edge shapes of tests/test_darboux_object_gpu.py cross): point chunks per object =
ceil(N / 1 024) within [8, 64] (some empty below N = 50); sweeps of 1 024 points; 128 workgroups share an object's rows
(2 per frame), 8 rows per workgroup and pass as shipped, so a pass holds 1 024 rows = 512 frames."""
import numpy as np

SCORE_TOL = 1e-4            # tests/local_search_ref.py: the bar for this same score (its scale is 1)
SWEEP = 1024                # csrc/darboux_object.hip: 256 lanes x DO_U
CHUNK_POINTS = 1024         # DO_CHUNK_POINTS
MIN_CHUNKS = 8              # DO_MIN_CHUNKS
GRID_X = 128                # DO_GX
PASS_ROWS = 1024            # DO_GX * DO_SLOTS (as shipped: 4 x 12 x 3)
OUTCOMES = ("slab", "back", "finger", "few", "all", "some", "fail")
NEAR = 1e-5
MIN_GAP = 1e-3
MIN_MINOR = 0.1
DEGENERATE = 1e-12
FLIP = np.array([1.0, -1.0, -1.0])

SABOTAGES = ("shift_order", "no_last_shift", "divide_by_passed", "round", "no_truncation", "inv_sign", "gate_order",
             "back_nonstrict", "band_half", "z_window", "no_abs", "slab_of_depth0", "back_ignored")


def _f32(v):
    return float(np.float32(v))


def constants(cfg):
    """The fp32 values the kernels and the reference compare against, as float64."""
    tb = cfg.tables()
    c = {k: tb[k].numpy().astype(np.float64) for k in tb}
    c.update(hbw=_f32(cfg.half_bottom_width), hbs=_f32(cfg.half_bottom_space), m=_f32(cfg.back_collision_margin),
             back_thr=_f32(cfg.back_collision_threshold), fing_thr=_f32(cfg.finger_collision_threshold),
             min_points=_f32(cfg.close_region_min_points), nd=_f32(cfg.neighbor_depth),
             slab_thr=_f32(cfg.num_points_threshold))
    return c


def frames64(P, Nn, radius=0.01, min_neighbours=5, dtype=np.float64, projector=False, rows=None):
    """P, Nn (N, 3) fp32 -> dict of `frames`, `inv_frames` (N, 3, 3), `count`, `flags` (1 estimated, 2 degenerate, 4
    few), `near`, `gap`, `minor_norm`.  dtype=np.float32 evaluates :73-91 in fp32 on the float64 neighbour set.
    projector=True is the SABOTAGE that builds the projector I - n n^T the view class builds.  rows: only these rows
    are computed (the others stay zero)."""
    p = np.asarray(P, np.float64)
    nrm = np.asarray(Nn).astype(dtype)
    N = len(p)
    r2 = float(np.float32(radius) * np.float32(radius))
    out = {"frames": np.zeros((N, 3, 3), dtype), "inv_frames": np.zeros((N, 3, 3), dtype),
           "count": np.zeros(N, np.int32), "flags": np.zeros(N, np.int32), "near": np.zeros(N, bool),
           "gap": np.zeros(N), "minor_norm": np.zeros(N)}
    for i in (range(N) if rows is None else rows):
        if not np.isfinite(p[i]).all():
            out["flags"][i] = 2
            continue
        d2 = ((p - p[i]) ** 2).sum(1)
        idx = np.nonzero(d2 < r2)[0]
        out["near"][i] = bool((np.abs(d2 - r2) < NEAR * r2).any())
        out["count"][i] = len(idx)
        if not np.isfinite(nrm[idx]).all():
            out["flags"][i] = 2
            continue
        if len(idx) < min_neighbours:                                          # :75-78
            out["flags"][i] = 4
            continue
        normal = np.mean(nrm[idx], axis=0)                                     # :73
        length = np.linalg.norm(normal)
        if not length >= 1e-12:
            out["flags"][i] = 2
            continue
        normal = normal / length                                               # :74
        if projector:
            M = np.eye(3, dtype=dtype) - normal[:, None] @ normal[None]
        else:
            M = np.eye(3, dtype=dtype) - normal.T @ normal                     # :80 -- a scalar off every entry
        c = np.mean(M @ nrm[idx].T, axis=1, keepdims=True)                     # :81
        d = nrm[idx].T - c                                                     # :82
        cov = d @ d.T                                                          # :83
        w, v = np.linalg.eigh(cov)                                             # :84
        minor = v[:, 0] - v[:, 0] @ normal.T * np.squeeze(normal)              # :86
        norm = np.linalg.norm(minor)
        out["gap"][i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
        out["minor_norm"][i] = norm
        if not norm * norm >= DEGENERATE:
            out["flags"][i] = 2
            continue
        minor = minor / norm                                                   # :87
        if minor[np.abs(minor).argmax()] < 0:                                  # the sign rule of `estimate_frames`
            minor = -minor
        principal = np.cross(minor, np.squeeze(normal))                        # :88
        out["frames"][i] = np.stack([-normal, -principal, minor], axis=1)      # :90
        out["inv_frames"][i] = np.stack([normal, principal, minor], axis=1)    # :91
        out["flags"][i] = 1
    return out


def frames_decided(y):
    """The estimated frames an fp32 implementation is held to (tests/darboux_ref.py `decided`)."""
    return (y["flags"] == 1) & ~y["near"] & (y["gap"] >= MIN_GAP) & (y["minor_norm"] >= MIN_MINOR)


def flip_distance(a, b):
    """max |a - b| per frame, modulo the joint flip of the y and z columns."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.minimum(np.abs(a - b).max((-1, -2)), np.abs(a * FLIP - b).max((-1, -2)))


def _near(v, faces, tol):
    out = np.zeros(v.shape, bool)
    for f in faces:
        out |= np.abs(v - f) < tol
    return out


def local64(P, R, p):
    """Global -> local of decision 4 in float64: R^T (P - p), exact products of the fp32 inputs.  -> (3, N)."""
    return (np.asarray(R, np.float64).T @ (np.asarray(P, np.float64) - np.asarray(p, np.float64)).T)


def grade64(P, Nn, frames, inv_frames, cfg, index=None, eps=0.0, sabotage=None, count=None):
    """P, Nn (N, 3) fp32; frames, inv_frames (F, 3, 3) fp32; index (F,) the point of each frame (default arange(F));
    count: only the first `count` points are points.  -> dict: `search_score` (F, 2, L, T) int64, `antipodal_score`
    float64, `counts` (F, 2, L, T, S, 3), `slab_count` (F, 2, L), `fail` (F, 2), `decided` (F, 2, L, T) bool,
    `outcome` (F, 2, L, T) index into OUTCOMES, `fractional` (F, 2, L, T): only some shifts passed."""
    k = constants(cfg)
    L, T, S = cfg.shape
    order = list(range(S))
    if sabotage == "shift_order":
        order = list(np.argsort(np.asarray(cfg.shift_search, np.float64), kind="stable"))
    zlo, zhi = k["zlo"], k["zhi"]
    if sabotage == "z_window":
        zlo, zhi = np.full(S, -_f32(cfg.half_hand_thickness)), np.full(S, _f32(cfg.half_hand_thickness))
    n_pts = len(P) if count is None else int(count)
    P64 = np.asarray(P, np.float64)[:n_pts]
    N64 = np.asarray(Nn, np.float64)[:n_pts]
    F = len(frames)
    index = np.arange(F) if index is None else np.asarray(index)
    out = {"search_score": np.zeros((F, 2, L, T), np.int64), "antipodal_score": np.zeros((F, 2, L, T)),
           "counts": np.zeros((F, 2, L, T, S, 3), np.int64), "slab_count": np.zeros((F, 2, L), np.int64),
           "fail": np.zeros((F, 2), bool), "decided": np.ones((F, 2, L, T), bool),
           "outcome": np.full((F, 2, L, T), 6, np.int64), "fractional": np.zeros((F, 2, L, T), bool)}
    if sabotage == "no_truncation":
        out["search_score"] = np.zeros((F, 2, L, T))
    zmax = max(abs(float(np.float32(cfg.half_hand_thickness + abs(float(d))))) for d in cfg.shift_search)
    r2lim = (k["hbw"] ** 2 + zmax ** 2) * 1.01 + 1e-6
    f32 = np.float32
    for f in range(F):
        for dr in range(2):
            R = np.asarray((inv_frames if dr else frames)[f], np.float64)
            if sabotage == "inv_sign" and dr:
                R = -np.asarray(frames[f], np.float64)
            i = int(index[f])
            ok = 0 <= i < n_pts and bool(np.isfinite(R).all()) and bool(np.isfinite(P64[i]).all())
            if not ok or np.abs(R).mean() < 1e-6:                            # :136, decision 2
                out["fail"][f, dr] = True
                continue
            x, y, z = local64(P64, R, P64[i])
            nl = R.T @ N64.T                                                 # :146
            near_x = np.stack([_near(x, (k["lo"][d], k["hi"][d]), eps) for d in range(L)])
            slab = np.stack([(x < k["hi"][d]) & (x > k["lo"][d]) for d in range(L)])          # :150-151
            n_slab, a_slab = slab.sum(1), near_x.sum(1)
            out["slab_count"][f, dr] = n_slab
            keep = (slab | near_x).any(0) & (y * y + z * z < r2lim)
            x, y, z, ny, nz = x[keep], y[keep], z[keep], nl[1][keep], nl[2][keep]
            slab, near_x = slab[:, keep], near_x[:, keep]
            for t in range(T):
                c, s = k["cos"][t], k["sin"][t]
                yy, zz = c * y + s * z, -s * y + c * z                       # config.py:79-82
                an = c * ny + s * nz if sabotage == "no_abs" else np.abs(c * ny + s * nz)      # :241-244
                near_yz = _near(yy, (k["hbw"], -k["hbw"], k["hbs"], -k["hbs"]), eps) | \
                    _near(zz, tuple(k["zlo"]) + tuple(k["zhi"]), eps)
                wide_yz = (np.abs(yy) < k["hbw"] + eps) & (zz < k["zhi"].max() + eps) & (zz > k["zlo"].min() - eps)
                zin = [(zz < zhi[q]) & (zz > zlo[q]) for q in range(S)]     # :183-184
                in_y = (yy < k["hbw"]) & (yy > -k["hbw"])
                fing_y = ((yy < k["hbw"]) & (yy > k["hbs"])) | ((yy > -k["hbw"]) & (yy < -k["hbs"]))   # :173-176
                close_y = (yy < k["hbs"]) & (yy > -k["hbs"])                                           # :196-198
                for d in range(L):
                    xs = x - k["depth"][d]
                    sl = slab[0] if sabotage == "slab_of_depth0" else slab[d]
                    wide = (slab[d] | near_x[d]) & wide_yz
                    dec = not (wide & (near_x[d] | near_yz | (np.abs(xs + k["m"]) < eps))).any()
                    dec &= bool((n_slab[d] - a_slab[d] >= k["slab_thr"]) or (n_slab[d] + a_slab[d] < k["slab_thr"]))
                    back_xy = sl & in_y & (xs < -k["m"])                     # :169-171
                    for q in range(S):
                        out["counts"][f, dr, d, t, q] = ((back_xy & zin[q]).sum(), (sl & fing_y & zin[q]).sum(),
                                                         (sl & close_y & zin[q]).sum())
                    if n_slab[d] < k["slab_thr"]:                            # :153
                        out["outcome"][f, dr, d, t] = 0
                        out["decided"][f, dr, d, t] = dec
                        continue
                    temp_s, temp_a = f32(0), 0.0                             # decision 1
                    crpn, single = f32(0), 0.0
                    total, passed, why = 0, 0, 1
                    for q in order:                                          # :181
                        nb, nf, nc = (int(v) for v in out["counts"][f, dr, d, t, q])
                        hit = nb >= k["back_thr"] if sabotage == "back_nonstrict" else nb > k["back_thr"]
                        if hit and sabotage != "back_ignored":               # :188
                            why = 1
                            continue
                        if nf > k["fing_thr"]:                               # :193
                            why = 2
                            continue
                        if sabotage != "gate_order":
                            crpn = f32(nc)                                   # :200
                        if nc < k["min_points"] or nc == 0:                  # :201
                            why = 3
                            continue
                        crpn = f32(nc)
                        sel = sl & close_y & zin[q]
                        cy, ca = yy[sel], an[sel]
                        left_y, right_y = cy.max(), cy.min()                 # :235-236
                        dep = min((left_y - right_y) / (2 if sabotage == "band_half" else 3), k["nd"])   # :237
                        lthr, rthr = left_y - dep, right_y + dep
                        il, ir = cy > lthr, cy < rthr                        # :239-240
                        dec &= not _near(cy, (lthr, rthr), eps).any()
                        with np.errstate(invalid="ignore", divide="ignore"):
                            single = (ca[il].sum() / il.sum()) * (ca[ir].sum() / ir.sum())     # :246
                        temp_a = temp_a + single / 3                         # :212
                        temp_s = f32(temp_s + f32(crpn / f32(3)))            # :213, fp32 in shift order
                        total += nc
                        passed += 1
                    if sabotage == "divide_by_passed" and passed:
                        temp_s, temp_a = f32(total / passed), temp_a * 3 / passed
                    if sabotage == "no_last_shift":
                        search, anti = float(temp_s), temp_a
                    else:
                        search = float(min(temp_s, crpn))                    # :215
                        anti = np.nan if np.isnan(temp_a) or np.isnan(single) else min(temp_a, single)   # :218
                    if sabotage == "round":
                        search = np.rint(search)
                    out["search_score"][f, dr, d, t] = search if sabotage == "no_truncation" else int(search)
                    out["antipodal_score"][f, dr, d, t] = anti
                    out["outcome"][f, dr, d, t] = 4 if passed == S else 5 if passed else why
                    out["fractional"][f, dr, d, t] = 0 < passed < S
                    out["decided"][f, dr, d, t] = dec and not np.isnan(anti)
    return out


def lattice_cloud(rng, n, step=1.0 / 2048, half=(40, 60, 30)):
    """n distinct points on a lattice of `step` within +-half steps per axis, unit-ish normals along +-y with |n.y| a
    multiple of 1/8: local coordinates in an axis-aligned frame at a lattice point are exact in fp32.
    -> (P (n, 3), Nn (n, 3)) fp32."""
    seen, pts = set(), []
    while len(pts) < n:
        c = tuple(int(rng.integers(-h, h + 1)) for h in half)
        if c not in seen:
            seen.add(c)
            pts.append(c)
    P = (np.array(pts, np.float64) * step).astype(np.float32)
    Nn = np.zeros((n, 3), np.float32)
    Nn[:, 1] = np.where(P[:, 1] >= 0, 1.0, -1.0) * rng.integers(1, 9, n) / 8.0
    Nn[:, 0] = rng.integers(-2, 3, n) / 8.0
    return P, Nn


def axis_frames(rng, n):
    """n axis-aligned rotations (signed permutations with determinant +1) and their opposite frames [-x, -y, z]."""
    perms = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]
    Fr = np.zeros((n, 3, 3), np.float32)
    for f in range(n):
        pm = perms[int(rng.integers(6))]
        sg = rng.choice([-1.0, 1.0], 3)
        M = np.zeros((3, 3))
        for c in range(3):
            M[pm[c], c] = sg[c]
        if np.linalg.det(M) < 0:
            M[:, 2] = -M[:, 2]
        Fr[f] = M
    return Fr, (Fr * np.array([-1.0, -1.0, 1.0], np.float32)).astype(np.float32)
