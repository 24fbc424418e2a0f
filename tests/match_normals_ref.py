"""Float64 yardstick of the normal matching (`postprocess.match_normals`, csrc/match_normals.hip): the reference's
`TorchSingleViewPointCloud._find_normal` (data_gen/pcd_classes/torch_single_view_point_cloud.py:135-150) restated in
numpy on one scene, with a brute-force hybrid search (the max_nn nearest of the points with d^2 < r^2, ranked by
(d^2, index)) in place of the kd-tree, and open3d's `normalize_normals` and `orient_normals_towards_camera_location`
as include/s4g_ops.h states them.

`decided` marks the queries on which an fp32 implementation picks the same set as a float64 kd-tree: no scene point
within NEAR (relative) of the sphere, and where the cap cuts, the (max_nn + 1)-th squared distance beyond the max_nn-th
by more than NEAR * r^2.  The fp32 differences of nearby fp32 coordinates are exact, so the fp32 d^2 is within about
2e-7 relative of the float64 one: far inside NEAR."""
import numpy as np

NEAR = 1e-5
CAPPED, EMPTY, CANCELLED, NONFINITE = 1, 2, 4, 8


def normals64(cloud, scene, scene_normals, camera, radius, max_nn, dtype=np.float64):
    """cloud (3, N), scene, scene_normals (3, M) fp32, camera (3,) or None.  -> dict of `normals` (N, 3) float64,
    `count`, `flags`, `in_radius` (N,), `mean_norm` (N,) the length of the unnormalised mean, `near` and `cap_tie`
    (what `decided` reads), `flipped` (the orientation turned the normal) and `kept` (N, max_nn) the kept scene indices
    in rank order padded with -1.  dtype=np.float32 accumulates the mean in fp32 on the float64 neighbour set.
    d^2 is evaluated in float64; on `lattice` inputs it equals the fp32 one."""
    q = np.asarray(cloud, np.float32).astype(np.float64).T
    p = np.asarray(scene, np.float32).astype(np.float64).T
    nrm = np.asarray(scene_normals, np.float32).T
    N, r2 = q.shape[0], float(radius) ** 2
    out = {"normals": np.zeros((N, 3)), "count": np.zeros(N, np.int32), "flags": np.zeros(N, np.int32),
           "in_radius": np.zeros(N, np.int64), "mean_norm": np.zeros(N), "near": np.zeros(N, bool),
           "cap_tie": np.zeros(N, bool), "flipped": np.zeros(N, bool), "kept": np.full((N, max_nn), -1, np.int64)}
    cam = None if camera is None else np.asarray(camera, np.float32).astype(np.float64)
    for i in range(N):
        flag = 0
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = ((p - q[i]) ** 2).sum(1)
            inside = np.nonzero(d2 < r2)[0]                      # NaN and inf compare false: never a neighbour
            out["near"][i] = bool((np.abs(d2 - r2) < NEAR * r2).any())
        order = inside[np.lexsort((inside, d2[inside]))]         # by d^2, the lower index winning a tie
        kept = order[:max_nn]
        if len(order) > max_nn:
            flag |= CAPPED
            out["cap_tie"][i] = d2[order[max_nn]] - d2[order[max_nn - 1]] <= NEAR * r2
        k = len(kept)
        out["in_radius"][i], out["count"][i] = len(order), k
        out["kept"][i, :k] = kept
        q_ok = bool(np.isfinite(q[i]).all())
        n = np.array([0.0, 0.0, 1.0])                            # the mean of nothing is NaN: normalize_normals' (0, 0, 1)
        orient = cam is not None
        if not q_ok:
            flag |= NONFINITE
        if k == 0:
            flag |= EMPTY
        elif not np.isfinite(nrm[kept]).all():
            flag |= NONFINITE
            n = np.full(3, np.nan)
            orient = False
        else:
            m = nrm[kept].astype(dtype).sum(0, dtype=dtype) / dtype(k)
            m = m.astype(np.float64)
            length = float(np.sqrt((m * m).sum()))
            out["mean_norm"][i] = length
            if length > 0.0:
                n = m / length
            else:
                n = np.zeros(3)
                flag |= CANCELLED
        if orient:
            with np.errstate(invalid="ignore", over="ignore"):
                ref = cam - q[i]
            if np.isfinite(ref).all():
                if not n.any():
                    rl = float(np.sqrt((ref * ref).sum()))
                    n = ref / rl if rl > 0.0 else np.array([0.0, 0.0, 1.0])
                elif float(n[0] * ref[0] + n[1] * ref[1] + n[2] * ref[2]) < 0.0:
                    n = -n
                    out["flipped"][i] = True
        out["normals"][i] = n
        out["flags"][i] = flag
    return out


def decided(y):
    """The queries of `normals64`'s result whose neighbour set an fp32 implementation is held to."""
    return ~y["near"] & ~y["cap_tie"]


def lattice(points, step=1.0 / 64):
    """Integer lattice coordinates (.., 3) -> fp32 (3, n) on a power-of-two lattice: with radius 0.25 every squared
    distance between such points is exact in fp32 (and equal to the float64 one)."""
    return (np.asarray(points, np.float64).reshape(-1, 3) * step).astype(np.float32).T.copy()


def in_radius32(cloud, scene, radius):
    """The number of scene points inside the radius of every query by the kernel's own fp32 rule: the subtraction, the
    squares and the sum ((dx^2 + dy^2) + dz^2) each rounded to fp32, against the fp32 product radius * radius; strict."""
    q, p = np.asarray(cloud, np.float32).T, np.asarray(scene, np.float32).T
    r = np.float32(radius)
    r2 = np.float32(r * r)
    out = np.zeros(q.shape[0], np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(q.shape[0]):
            d = p - q[i]
            s = d * d
            out[i] = int((((s[:, 0] + s[:, 1]) + s[:, 2]) < r2).sum())
    return out


def edge_cases():
    """name -> (cloud, scene, scene_normals, camera, max_nn, expect): the exact constructions the kernel is held to as
    well (tests/test_match_normals_gpu.py) and the yardstick's self-test.  Coordinates on a 1/64 lattice with radius 0.25 = 16 steps: every d^2 is
    exact in fp32.  expect: dict of count / flags / normals (None: the yardstick alone says)."""
    L = lattice
    up, down, side = [0, 0, 1], [0, 0, -1], [1, 0, 0]
    cases = {}

    def ring(k):             # k points inside the radius, at most 13 steps away
        return [[1 + (i % 12), i // 12, 0] for i in range(k)]

    def case(name, q, pts, nrm, cam, max_nn, **expect):
        cases[name] = (L(q), L(pts), np.asarray(nrm, np.float32).reshape(-1, 3).T.copy(),
                       None if cam is None else np.asarray(cam, np.float32), max_nn, expect)

    cam = [0.0, 0.0, 4.0]
    # a point at exactly r (16 steps) is excluded, one at 15 steps is in
    case("at r", [0, 0, 0], [[16, 0, 0], [15, 0, 0]], [side, up], cam, 30, count=[1], flags=[0], normals=[up])
    for max_nn in (1, 5, 30, 64):
        pts = ring(max_nn)
        far = [[0, 15, 0]]                                                 # farther than every ring point
        case("k = max_nn = %d" % max_nn, [0, 0, 0], pts, [up] * max_nn, cam, max_nn,
             count=[max_nn], flags=[0], normals=[up])
        case("k = max_nn + 1 = %d" % (max_nn + 1), [0, 0, 0], pts + far, [up] * max_nn + [side], cam, max_nn,
             count=[max_nn], flags=[CAPPED], normals=[up])
    # an exact tie across the cap: (3, 4, 0) and (5, 0, 0) are both 5 steps away; the lower index wins
    case("tie, low index first", [0, 0, 0], [[1, 0, 0], [3, 4, 0], [5, 0, 0]], [up, up, side], cam, 2,
         count=[2], flags=[CAPPED], normals=[up])
    case("tie, low index last", [0, 0, 0], [[1, 0, 0], [5, 0, 0], [3, 4, 0]], [up, side, up], cam, 2,
         count=[2], flags=[CAPPED], normals=[[2 ** -0.5, 0, 2 ** -0.5]])
    case("k = 0", [0, 0, 0], [[40, 0, 0]], [side], cam, 30, count=[0], flags=[EMPTY], normals=[up])
    case("k = 0, camera below", [0, 0, 0], [[40, 0, 0]], [side], [0, 0, -4.0], 30, count=[0], flags=[EMPTY],
         normals=[down])
    case("cancel", [0, 0, 0], [[1, 0, 0], [2, 0, 0]], [side, [-1, 0, 0]], [0, 3.0, 4.0], 30,
         count=[2], flags=[CANCELLED], normals=[[0, 0.6, 0.8]])
    case("cancel, no camera", [0, 0, 0], [[1, 0, 0], [2, 0, 0]], [side, [-1, 0, 0]], None, 30,
         count=[2], flags=[CANCELLED], normals=[[0, 0, 0]])
    case("n . ref == 0", [0, 0, 0], [[1, 0, 0]], [side], cam, 30, count=[1], flags=[0], normals=[side])
    case("n . ref < 0", [0, 0, 0], [[1, 0, 0]], [down], cam, 30, count=[1], flags=[0], normals=[up])
    case("camera=None", [0, 0, 0], [[1, 0, 0]], [down], None, 30, count=[1], flags=[0], normals=[down])
    case("camera at the query", [[0, 0, 0], [64, 0, 0]], [[1, 0, 0], [2, 0, 0], [65, 0, 0]], [side, [-1, 0, 0], down],
         [0, 0, 0], 30, count=[2, 1], flags=[CANCELLED, 0], normals=[up, down])
    case("M = 1", [[0, 0, 0], [3, 0, 0]], [[0, 0, 0]], [[0, 0, 2]], cam, 30, count=[1, 1], flags=[0, 0],
         normals=[up, up])
    return cases
