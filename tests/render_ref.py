"""float64 numpy yardstick of `render_views` (csrc/render_views.hip; contract: include/s4g_ops.h,
s4g_render_views_f32): data_gen/render/cycles_render.py:25-36, 118-153 restated without Blender.  Written from the
statements of the contract, not from the kernel: every ray is tested against EVERY triangle, no culling structure.

Every operation is elementwise numpy in the order the contract writes it (sums left to right), so on inputs where
every product is exact the result is the kernel's bit for bit.  Elsewhere the two may differ in the last bits of a
double; `decided` marks the pixels where that cannot change a decision:
  * no triangle in front of the camera (Tn / det > 0) has the ray within 1e-9 (barycentric, min(U, V, det - U - V) /
    |det|) of one of its edges, and
  * the two nearest hits differ by more than 1e-9 relative.
Both sides compute in double (rounding ~1e-16), so 1e-9 leaves seven orders of magnitude.

`sabotage=` names one deliberate misreading of the reference (tests/test_render_ref.py shows that each changes the
result: the fixture pins every one of these choices)."""
from collections import namedtuple

import numpy as np

# cycles_render.py:14-19: (x, y, z, qw, qx, qy, qz)
CAMERA_POSE = ((0.8, 0, 1.7, 0.948, 0, 0.317, 0),
               (-0.8, 0, 1.6, -0.94, 0, 0.342, 0),
               (0.0, 0.75, 1.7, 0.671, -0.224, 0.224, 0.671),
               (0.0, -0.75, 1.6, -0.658, -0.259, -0.259, 0.658))
WIDTH, HEIGHT, FX, FY, CX, CY, MAX_DEPTH = 640, 480, 700.0, 700.0, 320.0, 240.0, 5.0
EPS = 1e-9

SABOTAGES = ("backface", "exclusive", "first", "higher_tie", "planar_range", "rows_from_top", "z_not_negated",
             "corners", "xyzw", "rt", "le_max", "no_normalise")

Result = namedtuple("Result", "range triangle decided kept points noisy pixels")
Intrinsics = namedtuple("Intrinsics", "fx fy cx cy max_depth H W")


def intrinsics(scale=1.0):
    """The reference's pinhole, or the same field of view at `scale` times the resolution."""
    return Intrinsics(FX * scale, FY * scale, CX * scale, CY * scale, MAX_DEPTH, int(round(HEIGHT * scale)),
                      int(round(WIDTH * scale)))


def quat2mat(q):
    """transforms3d.quaternions.quat2mat for (w, x, y, z), float64."""
    w, x, y, z = (float(v) for v in q)
    nq = w * w + x * x + y * y + z * z
    if nq < np.finfo(np.float64).eps:
        return np.eye(3)
    s = 2.0 / nq
    X, Y, Z = x * s, y * s, z * s
    wX, wY, wZ, xX, xY, xZ, yY, yZ, zZ = w * X, w * Y, w * Z, x * X, x * Y, x * Z, y * Y, y * Z, z * Z
    return np.array([[1.0 - (yY + zZ), xY - wZ, xZ + wY],
                     [xY + wZ, 1.0 - (xX + zZ), yZ - wX],
                     [xZ - wY, yZ + wX, 1.0 - (xX + yY)]], dtype=np.float64)


def camera(pose, sabotage=None):
    """pose (x, y, z, qw, qx, qy, qz) -> (R (3, 3), c (3,)) float64, camera to world."""
    pose = [float(v) for v in pose]
    q = pose[3:7]
    if sabotage == "xyzw":
        q = [q[3], q[0], q[1], q[2]]
    return quat2mat(q), np.array(pose[:3], dtype=np.float64)


def cam12(R, c):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(c, np.float64).reshape(3)])


def _rays(pixels, K, sabotage):
    row, col = pixels // K.W, pixels % K.W
    half = 0.0 if sabotage == "corners" else 0.5
    x = col.astype(np.float64) + half
    y = (K.H - 1 - row if sabotage == "rows_from_top" else row).astype(np.float64) + half
    return (x - K.cx) / K.fx, (y - K.cy) / K.fy


def unproject(range32, hit, pixels, R, c, K, noise=None, sabotage=None):
    """range32 (n,) fp32 ray lengths of `pixels` -> (kept (n,) bool, points (n, 3) fp32, noisy (n, 3) fp32 or None);
    rows that are not kept hold NaN."""
    rx, ry = _rays(pixels, K, sabotage)
    nor = np.sqrt(rx * rx + ry * ry + 1.0)
    if sabotage == "no_normalise":
        dx, dy, dz = rx, ry, np.ones_like(rx)
    else:
        dx, dy, dz = rx / nor, ry / nor, 1.0 / nor
    r = np.asarray(range32, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        kept = hit & ((r * dz <= K.max_depth) if sabotage == "le_max" else (r * dz < K.max_depth))
    M = R.T if sabotage == "rt" else R

    def world(rr):
        with np.errstate(invalid="ignore", over="ignore"):
            x, y, z = rr * dx, rr * dy, rr * dz
            if sabotage != "z_not_negated":
                z = -z
            out = np.stack([M[i, 0] * x + M[i, 1] * y + M[i, 2] * z + c[i] for i in range(3)], axis=1)
            out = out.astype(np.float32)
        out[~kept] = np.nan
        return out

    noisy = None if noise is None else world(r * np.asarray(noise, np.float64))
    return kept, world(r), noisy


def camera_frame(tri, R, c):
    """(T, 3, 3) fp32 world triangles -> the per-triangle terms in double: v0, e1, e2, Q (T, 3) and Tn (T,)."""
    d = np.asarray(tri, np.float32).reshape(-1, 3, 3).astype(np.float64) - c
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.stack([R[0, i] * d[..., 0] + R[1, i] * d[..., 1] + R[2, i] * d[..., 2] for i in range(3)], axis=-1)
        v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        Q = np.stack([-(v0[:, 1] * e1[:, 2] - v0[:, 2] * e1[:, 1]), -(v0[:, 2] * e1[:, 0] - v0[:, 0] * e1[:, 2]),
                      -(v0[:, 0] * e1[:, 1] - v0[:, 1] * e1[:, 0])], axis=1)
        Tn = e2[:, 0] * Q[:, 0] + e2[:, 1] * Q[:, 1] + e2[:, 2] * Q[:, 2]
    return v0, e1, e2, Q, Tn


def render_ref(tri, R, c, K, noise=None, pixels=None, tri_count=None, sabotage=None, budget=2_000_000):
    """One view.  tri (T, 3, 3) fp32; R, c from `camera`; K an `Intrinsics`; pixels: the pixel indices to render
    (default: all, ascending); noise: multipliers per rendered pixel.  -> `Result` over those pixels: range (fp32, +inf
    on a miss), triangle (int32, -1), decided, kept, points / noisy (n, 3) fp32 with NaN where not kept."""
    assert sabotage is None or sabotage in SABOTAGES, sabotage
    tri = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    if tri_count is not None:
        tri = tri[:max(0, min(int(tri_count), len(tri)))]
    T = len(tri)
    pixels = np.arange(K.H * K.W, dtype=np.int64) if pixels is None else np.asarray(pixels, np.int64)
    n = len(pixels)
    rx_all, ry_all = _rays(pixels, K, sabotage)
    best_t = np.full(n, np.inf)
    best_i = np.full(n, -1, np.int32)
    decided = np.ones(n, bool)
    if T:
        v0, e1, e2, Q, Tn = camera_frame(tri, R, c)
        step = max(1, budget // T)
        for s in range(0, n, step):
            rx, ry = rx_all[s:s + step, None], ry_all[s:s + step, None]
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                px = ry * e2[:, 2] + e2[:, 1]                       # P = r x e2 with r.z = -1
                py = -e2[:, 0] - rx * e2[:, 2]
                pz = rx * e2[:, 1] - ry * e2[:, 0]
                det = e1[:, 0] * px + e1[:, 1] * py + e1[:, 2] * pz
                U = -(v0[:, 0] * px + v0[:, 1] * py + v0[:, 2] * pz)
                V = rx * Q[:, 0] + ry * Q[:, 1] - Q[:, 2]
                W3 = U + V
                if sabotage == "exclusive":
                    pos = (det > 0) & (U > 0) & (V > 0) & (W3 < det) & (Tn > 0)
                    neg = (det < 0) & (U < 0) & (V < 0) & (W3 > det) & (Tn < 0)
                else:
                    pos = (det > 0) & (U >= 0) & (V >= 0) & (W3 <= det) & (Tn > 0)
                    neg = (det < 0) & (U <= 0) & (V <= 0) & (W3 >= det) & (Tn < 0)
                fin = np.isfinite(det) & np.isfinite(U) & np.isfinite(V) & np.isfinite(Tn)
                hit = (pos if sabotage == "backface" else (pos | neg)) & fin
                tq = Tn / det
                t = np.where(hit, tq, np.inf)
                rows = np.arange(t.shape[0])
                if sabotage == "first":
                    bi = np.argmax(hit, axis=1)
                elif sabotage == "higher_tie":
                    bi = T - 1 - np.argmin(t[:, ::-1], axis=1)
                else:
                    bi = np.argmin(t, axis=1)                       # the first of equal minima: the lowest index
                bt = t[rows, bi]
                found = np.isfinite(bt)
                # decided: no edge of a triangle in front within EPS of the ray, nearest two hits apart
                front = fin & (det != 0) & (tq > 0)
                sg = np.sign(det)
                margin = np.minimum(np.minimum(sg * U, sg * V), sg * (det - U - V)) / np.abs(det)
                edge = (front & (np.abs(margin) <= EPS)).any(axis=1)
                t2 = t.copy()
                t2[rows, bi] = np.inf
                bt2 = t2.min(axis=1)
                close = found & np.isfinite(bt2) & (bt2 - bt <= EPS * np.abs(bt))
            best_t[s:s + step] = np.where(found, bt, np.inf)
            best_i[s:s + step] = np.where(found, bi, -1)
            decided[s:s + step] = ~(edge | close)
    hit = best_i >= 0
    nor = np.sqrt(rx_all * rx_all + ry_all * ry_all + 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        r64 = best_t if sabotage == "planar_range" else best_t * nor
        range32 = np.where(hit, r64, np.inf).astype(np.float32)
    kept, points, noisy = unproject(range32, hit, pixels, R, c, K, noise, sabotage)
    return Result(range32, best_i, decided, kept, points, noisy, pixels)


def compact(res, P):
    """A full-view `Result` -> the kernel's compact outputs: points, noisy (3, P) fp32 (NaN from count on), pixel (P,)
    int32 (-1 from count on), count."""
    idx = np.nonzero(res.kept)[0]
    k = len(idx)
    pts = np.full((3, P), np.nan, np.float32)
    pts[:, :k] = res.points[idx].T
    nsy = None
    if res.noisy is not None:
        nsy = np.full((3, P), np.nan, np.float32)
        nsy[:, :k] = res.noisy[idx].T
    pix = np.full(P, -1, np.int32)
    pix[:k] = res.pixels[idx]
    return pts, nsy, pix, k


# ---- scenes ---------------------------------------------------------------------------------------------------------

def box_triangles(lo, hi):
    """The 12 triangles of an axis-aligned box, (12, 3, 3) fp32; faces in the order -x, +x, -y, +y, -z, +z, two
    triangles each, outward winding."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    p = np.array([[x0, y0, z0], [x1, y0, z0], [x0, y1, z0], [x1, y1, z0],
                  [x0, y0, z1], [x1, y0, z1], [x0, y1, z1], [x1, y1, z1]], dtype=np.float64)
    quads = ((0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6))
    tris = []
    for a, b, cc, d in quads:
        tris += [[p[a], p[b], p[cc]], [p[a], p[cc], p[d]]]
    return np.asarray(tris, np.float64).astype(np.float32)


TABLE_LO, TABLE_HI = (-0.38, -0.345, 0.70), (0.38, 0.345, 0.75)


def fixture_scene(g):
    """The fixture's scene, (T, 3, 3) fp32: the mesh moved by g["mesh_offset"] (float64 sum, rounded once), then the 12
    triangles of the table box."""
    v = (g["vertices"].astype(np.float64) + g["mesh_offset"].astype(np.float64)).astype(np.float32)
    mesh = v[g["faces"].astype(np.int64)]
    return np.concatenate([mesh, box_triangles(TABLE_LO, TABLE_HI)], axis=0)


def fixture_views(g):
    """[(name, R, c)] of the fixture's views: the four cameras, then camera 0 moved to 0.35 m from the object."""
    out = []
    for i in range(len(g["poses"])):
        R, c = camera(g["poses"][i])
        out.append(("view%d" % i, R, c))
    R, c = camera(g["close_pose"])
    out.append(("close", R, c))
    return out
