"""Float64 yardstick of the Darboux frame estimation (`postprocess.estimate_frames`, csrc/darboux.hip): the reference's
`TorchSingleViewPointCloud._estimate_frame` (data_gen/pcd_classes/torch_single_view_point_cloud.py:116-133) restated in
numpy on one scene, with a brute-force radius search in float64 (`d^2 < r^2`, the point itself included) in place of
the kd-tree, plus the quantities that say how well a frame is determined.

A frame's eigenvector is defined up to its sign: the frame's y and z columns flip together.  `flip_distance` compares
two frames modulo that flip.  `decided` marks the frames on which an fp32 implementation can be held to a bound:
no point within NEAR (relative) of r^2, the relative eigenvalue gap g = (l1 - l0) / l2 at least MIN_GAP (the error of
the eigenvector of l0 is the covariance's error over l2, divided by g) and the unnormalised minor axis no shorter than
MIN_MINOR (its normalisation divides the error by that length)."""
import numpy as np

NEAR = 1e-5
MIN_GAP = 1e-3
MIN_MINOR = 0.1
DEGENERATE = 1e-12          # squared norm of the unnormalised minor axis below which the frame is the zero frame
FLIP = np.array([1.0, -1.0, -1.0])


def sample_indices(cloud, sample_region):
    """:53 -- the ascending indices of the points with z > SAMPLE_REGION.  cloud (3, N)."""
    return np.nonzero(cloud[2] > sample_region)[0]


def frames64(cloud, normals, index, radius, min_neighbours=5, dtype=np.float64):
    """cloud, normals (3, N) fp32, index (F,) (negative: a padding row).  -> dict of `frames` (F, 3, 3) with the axes as
    columns (identity where count < min_neighbours, zero for padding and degenerate rows), `points` (F, 3), `count`,
    `estimated`, `degenerate`, `near` (a point within NEAR of the sphere), `eig` (F, 3) ascending, `gap` and
    `minor_norm`.  dtype=np.float32 evaluates lines :122-133 in fp32 on the float64 neighbour set."""
    p = cloud.astype(np.float64).T
    nrm = normals.astype(dtype).T
    F = len(index)
    r2 = float(radius) ** 2
    out = {"frames": np.zeros((F, 3, 3), dtype), "points": np.zeros((F, 3), np.float32), "count": np.zeros(F, np.int32),
           "estimated": np.zeros(F, bool), "degenerate": np.zeros(F, bool), "near": np.zeros(F, bool),
           "eig": np.zeros((F, 3)), "gap": np.zeros(F), "minor_norm": np.zeros(F)}
    for f, i in enumerate(index):
        if i < 0:
            continue
        out["points"][f] = cloud[:, i]
        d2 = ((p - p[i]) ** 2).sum(1)
        idx = np.nonzero(d2 < r2)[0]
        out["near"][f] = bool((np.abs(d2 - r2) < NEAR * r2).any())
        out["count"][f] = len(idx)
        if not (np.isfinite(p[i]).all() and np.isfinite(nrm[i]).all() and np.isfinite(nrm[idx]).all()):
            out["degenerate"][f] = True
            continue
        if len(idx) < min_neighbours:
            out["frames"][f] = np.eye(3)
            continue
        n = nrm[i:i + 1]
        M = np.eye(3, dtype=dtype) - n.T @ n                                   # :122
        c = np.mean(M @ nrm[idx].T, axis=1, keepdims=True)                     # :123
        d = nrm[idx].T - c                                                     # :124
        cov = d @ d.T                                                          # :125
        w, v = np.linalg.eigh(cov)                                             # :126
        minor = v[:, 0] - v[:, 0] @ n.T * np.squeeze(n)                        # :128
        norm = np.linalg.norm(minor)
        out["eig"][f] = w
        out["gap"][f] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
        out["minor_norm"][f] = norm
        if not norm * norm >= DEGENERATE:
            out["degenerate"][f] = True
            continue
        minor = minor / norm                                                   # :129
        principal = np.cross(minor, np.squeeze(n))                             # :130
        out["frames"][f] = np.stack([-n[0], -principal, minor], axis=1)        # :132
        out["estimated"][f] = True
    return out


def decided(y):
    """The estimated frames of `frames64`'s result that an fp32 implementation is held to."""
    return y["estimated"] & ~y["near"] & (y["gap"] >= MIN_GAP) & (y["minor_norm"] >= MIN_MINOR)


def count_decided(y):
    """The rows whose neighbour count is exact in fp32: no point within NEAR of the sphere."""
    return ~y["near"]


def flip_distance(a, b):
    """max |a - b| per frame, modulo the joint flip of the y and z columns.  a, b (..., 3, 3)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.minimum(np.abs(a - b).max((-1, -2)), np.abs(a * FLIP - b).max((-1, -2)))


def sign_agrees(a, b):
    """True where frame a is nearer to b than to b's flip."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max((-1, -2)) <= np.abs(a * FLIP - b).max((-1, -2))


def sign_rule_holds(frames, tol=1e-6):
    """The pinned sign: of the minor axis (column z) the component with the largest magnitude is positive -- checked
    where that component leads the next one by more than tol (the rule is applied to the unnormalised axis in the
    kernel's arithmetic, a tie within rounding may fall either way)."""
    z = np.asarray(frames, np.float64)[..., :, 2]
    a = np.abs(z)
    k = a.argmax(-1)
    top = np.take_along_axis(z, k[..., None], -1)[..., 0]
    second = np.sort(a, -1)[..., 1]
    return (top > 0) | (np.abs(top) - second <= tol)


def random_cloud(rng, N, radius, spread=2.5):
    """N points in a box of `spread` radii with noisy unit normals around +z, fp32: dense enough that most points have
    five neighbours, small enough that some do not."""
    cloud = rng.uniform(-0.5 * spread * radius, 0.5 * spread * radius, (3, N)).astype(np.float32)
    n = np.array([[0.0], [0.0], [1.0]]) + rng.normal(0, 0.3, (3, N))
    n /= np.linalg.norm(n, axis=0, keepdims=True)
    return cloud, n.astype(np.float32)


def parallel_patch():
    """Five points together whose normals (used as given, not unit) spread along x and y only, around point 0's normal
    +z: the covariance is diag(16, 16, 1) exactly, its smallest eigenvector is the normal itself and the minor axis
    vanishes -- a degenerate frame for point 0."""
    cloud = np.zeros((3, 5), np.float32)
    normals = np.array([[0, 0, 1], [2, 2, 0], [-2, -2, 0], [2, -2, 0], [-2, 2, 0]], np.float32).T.copy()
    return cloud, normals
