"""Float64 yardstick of the normal estimation (`postprocess.estimate_normals`, csrc/match_normals.hip): the reference's
`PointCloud.estimate_normals` (data_gen/pcd_classes/pointcloud.py:48-60) restated in numpy on one cloud -- open3d's
`estimate_normals(KDTreeSearchParamHybrid(radius, max_nn), fast_normal_computation=False)`, `normalize_normals` and
`orient_normals_towards_camera_location` as include/s4g_ops.h states them.

The neighbour set is EXACT, not approximate: it comes from the pinned fp32 squared distance (`d2_32`, the arithmetic of
`match_normals_ref.in_radius32`), the strict comparison against the fp32 product radius * radius and the tie rule
"(d^2, then the lower index)", so a kernel is held to the same set on every row.  The moments of the kept points about
the query, the covariance, `eigh` and the orientation are in float64; dtype=np.float32 restates all of them in fp32 (the
distance of that restatement from float64, times the relative gap, is the fixture's `margin`).

`variant` names one deliberate mistake (tests/test_normals_ref.py checks that each of them is caught)."""
import numpy as np

CAPPED, FEW, DEGENERATE, NONFINITE, PADDING = 1, 2, 4, 8, 16
FEW_BELOW = 3
VARIANTS = ("uncentred", "largest", "middle", "no cap", "cap by index", "non-strict", "doubled radius", "no self",
            "threshold 5", "no orientation", "inverted orientation", "tie reversed")


def d2_32(points, q):
    """fp32 squared distances of points (n, 3) fp32 to q (3,) fp32 by the kernel's rule: the subtraction, the squares and
    the sum ((dx^2 + dy^2) + dz^2) each rounded to fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = points - q
        s = d * d
        return (s[:, 0] + s[:, 1]) + s[:, 2]


def lead_positive(n):
    """The sign rule without a direction: the component of largest magnitude positive, the lowest axis on a tie."""
    a = np.abs(n)
    return -n if n[int(np.argmax(a))] < 0 else n        # argmax returns the first maximum


def normals_ref(cloud, camera, radius, max_nn, live=None, dtype=np.float64, variant=None, rows=None):
    """cloud (3, N) fp32, camera (3,) or None, live: the rows at or past it are padding (None: N).  -> dict of `normals`
    (N, 3) float64, `count`, `flags`, `inside` (N,) the points inside the radius, `gap` (N,) the relative gap g = (l1 -
    l0) / l2 of the float64 covariance (0 where no plane is fitted), `towards` (N,) n . (camera - p) / |camera - p| (0
    without a direction) and `kept` (N, max_nn) the kept indices in rank order padded with -1.  rows: the queries to
    evaluate (default all); the others keep zeros."""
    assert variant is None or variant in VARIANTS, variant
    p32 = np.ascontiguousarray(np.asarray(cloud, np.float32).T)
    N = p32.shape[0]
    n_live = N if live is None else min(max(int(live), 0), N)
    r = np.float32(radius)
    if variant == "doubled radius":
        r = np.float32(2) * r
    r2 = np.float32(r * r)
    finite = np.isfinite(p32).all(1)
    key_ok = finite & (np.arange(N) < n_live)
    key_index = np.nonzero(key_ok)[0]
    keys32 = p32[key_index]
    cam = None if camera is None else np.asarray(camera, np.float32).astype(np.float64)
    few_below = 5 if variant == "threshold 5" else FEW_BELOW
    out = {"normals": np.zeros((N, 3)), "count": np.zeros(N, np.int32), "flags": np.zeros(N, np.int32),
           "inside": np.zeros(N, np.int64), "gap": np.zeros(N), "towards": np.zeros(N),
           "kept": np.full((N, max_nn), -1, np.int64)}
    for i in (range(N) if rows is None else rows):
        if i >= n_live:
            out["flags"][i] = PADDING
            continue
        if not finite[i]:
            out["normals"][i] = (0.0, 0.0, 1.0)
            out["flags"][i] = NONFINITE
            continue
        d2 = d2_32(keys32, p32[i])
        with np.errstate(invalid="ignore"):
            inside = np.nonzero(d2 <= r2 if variant == "non-strict" else d2 < r2)[0]
        if variant == "no self":
            inside = inside[key_index[inside] != i]
        idx = key_index[inside]
        if variant == "cap by index":
            order = np.arange(len(idx))
        elif variant == "tie reversed":
            order = np.lexsort((-idx, d2[inside]))
        else:
            order = np.lexsort((idx, d2[inside]))            # by fp32 d^2, the lower index winning a tie
        kept = idx[order] if variant == "no cap" else idx[order][:max_nn]
        k = len(kept)
        flag = CAPPED if len(idx) > max_nn else 0
        out["inside"][i], out["count"][i] = len(idx), min(k, max_nn) if variant != "no cap" else k
        out["kept"][i, :min(k, max_nn)] = kept[:max_nn]
        n = np.array([0.0, 0.0, 1.0])
        if k < few_below:
            flag |= FEW
        elif (p32[kept] == p32[i]).all():
            flag |= DEGENERATE
        else:
            d = (p32[kept].astype(dtype) - p32[i].astype(dtype)).astype(dtype)      # exact for nearby fp32 points
            s1 = d.sum(0, dtype=dtype) / dtype(k)
            s2 = (d[:, :, None] * d[:, None, :]).sum(0, dtype=dtype) / dtype(k)
            cov = s2 if variant == "uncentred" else (s2 - np.outer(s1, s1)).astype(dtype)
            w, v = np.linalg.eigh(cov)
            zero = [a for a in range(3) if not cov[a].any()]
            if len(zero) == 1 and w[1] > 0:
                # an exactly zero row and column: that axis IS the eigenvector of the eigenvalue 0, the smallest one
                # where the other two are positive (LAPACK's tridiagonalisation may return it a rounding off)
                v = v.copy()
                v[:, 0] = np.eye(3, dtype=dtype)[zero[0]]
            col = {"largest": 2, "middle": 1}.get(variant, 0)
            e = v[:, col].astype(np.float64)
            length = float(np.sqrt((e * e).sum()))
            if np.isfinite(e).all() and length > 0.0:
                n = e / length
                if dtype == np.float64:
                    out["gap"][i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
            else:
                flag |= DEGENERATE
        dot = 0.0
        if cam is not None and variant != "no orientation":
            with np.errstate(invalid="ignore", over="ignore"):
                ref = (cam - p32[i].astype(np.float64)).astype(dtype).astype(np.float64)
            if np.isfinite(ref).all():
                dot = float(n[0] * ref[0] + n[1] * ref[1] + n[2] * ref[2])
                rl = float(np.sqrt((ref * ref).sum()))
                out["towards"][i] = dot / rl if rl > 0 else 0.0
        if dot != 0.0:
            flip = dot < 0.0
            n = -n if flip != (variant == "inverted orientation") else n
        else:
            n = lead_positive(n)
        out["normals"][i] = n
        out["flags"][i] = flag
    return out


def row_error(got, y):
    """The error of `got` (N, 3) against the yardstick result y, per row: sin(angle to y's normal) modulo the sign, and 2
    where the sign is wrong on a row whose sign the camera decides (|towards| > 1e-6)."""
    n64 = y["normals"]
    g = np.asarray(got, np.float64)
    cross = np.cross(g, n64)
    sin = np.sqrt((cross * cross).sum(1))
    dot = (g * n64).sum(1)
    sin = np.where(np.abs(dot) < 0.5, 1.0, sin)            # past 60 degrees the sine alone would fold back
    wrong_sign = (np.abs(y["towards"]) > 1e-6) & (dot < 0)
    return np.where(wrong_sign, 2.0, sin)


def bound(y, margin, factor=8.0):
    """Per row: factor * margin / g, on the rows a plane is fitted on (count >= 3); inf elsewhere and where g == 0."""
    g = y["gap"]
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.where(g > 0, factor * margin / g, np.inf)
    return np.where(y["count"] >= FEW_BELOW, b, np.inf)


def lattice_sheet(side=20, step=1.0 / 64, seed=7):
    """A bumpy sheet on a power-of-two lattice: x, y in [0, side), z in {0, 1, 2} steps, drawn from a fixed seed.  With
    a radius of 5 steps every squared distance is a small integer times step^2, exact in fp32: distance ties are
    everywhere, and points lie exactly on the sphere ((5, 0, 0), (3, 4, 0), (4, 0, 3), ...).  -> (3, side^2) fp32."""
    rng = np.random.RandomState(seed)
    xs, ys = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    z = rng.randint(0, 3, size=xs.shape)
    pts = np.stack([xs.ravel(), ys.ravel(), z.ravel()], 0).astype(np.float64) * step
    order = rng.permutation(pts.shape[1])                   # so that the index order is not the geometric one
    return pts[:, order].astype(np.float32).copy()
