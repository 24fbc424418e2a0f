"""Float64 yardstick of the baseline inputs (`postprocess.best_placement`, `close_regions`, `label_baseline_view`,
csrc/close_region.hip; the reference's `TorchBaseLineSingleViewPointCloud.finger_hand` :308-331 and
`close_region_projection` :334-393, data_gen/pcd_classes/torch_baseline_single_view_point_cloud.py).
TEST INFRASTRUCTURE ONLY.

  * `best64`        the fold over the L * T placements: the first score > 0 and > every earlier one; valid unless < 1e-4.
  * `g2l64`         LOCAL_TO_LOCAL_SEARCH[i] @ [R^T | -R^T p] in float64 (of the fp32 cos / sin / depth the reference forms).
  * `regions64`     per frame the CERTAIN members of the close region, the AMBIGUOUS ones (within `tol` of a face: an fp32
                    route may put them on either side) and the float64 local coordinates of both.
  * `projection64`  the 12-channel maps of an fp32 point set: voxel indices by the exact fp32 rule floor(c / unit) (an
                    fp32 division by the fp32 unit), everything after them in float64.
  * `near_voxel_face` / `pixel_mask`  the pixels a point within `vtol` of a voxel face can move between: two fp32 routes
                    to the local coordinates differ by about 1e-7 (the scene's coordinates are of size 1), so a point
                    that close to a face sits in one voxel for one route and in its neighbour for the other.

Every `sabotage=` is a deliberate mistake the tests must notice (tests/test_close_region_ref.py).

Loop structure of the kernels (what the edge shapes of tests/test_close_region_gpu.py cross): point chunks per scene =
ceil(N / 16 384) within [4, 64]; sweeps of 1 024 points; 32 workgroups share a scene's frames, 8 frames per workgroup and
pass, so a pass holds 256 frames; voxel tiles of one x slab by 32 y rows."""
import os

import numpy as np

TOL = 4e-6                   # the `tol` of tests/local_search_ref.py: the distance to a region face that counts as ambiguous
VTOL = 1e-6                  # a point this close to a voxel face may sit in the neighbouring voxel for another fp32 route
SWEEP_POINTS = 1024          # csrc/close_region.hip: 256 * CR_U
CHUNK_POINTS = 16384         # CR_CHUNK_POINTS (4 chunks at least: the count turns at N = 65 536 / 65 537)
FRAMES_PER_PASS = 256        # CR_GX * CR_SLOTS
ORDERS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))


def _f32(v):
    return float(np.float32(v))


def load_fixture():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_regions.npz")
    with np.load(path) as z:
        fx = {k: z[k] for k in z.files}
    R = int(fx["resolution"][0])
    V = int(fx["valid"].sum())
    maps = np.zeros(V * 12 * R * R, np.float32)
    maps[fx["map_nz_index"]] = fx["map_nz_value"]
    fx["maps"] = maps.reshape(V, 12, R, R)
    return fx


def best64(scores, sabotage=None):
    """scores (F, P) -> (index (F,) int64, -1 where invalid; score (F,); valid (F,) bool)."""
    scores = np.asarray(scores, np.float64)
    F, P = scores.shape
    index, best = np.full(F, -1, np.int64), np.zeros(F)
    for f in range(F):
        for i in range(P):
            s = scores[f, i]
            take = s >= best[f] and s > 0 if sabotage == "later_on_tie" else s > best[f]
            if take:
                best[f], index[f] = s, i
    valid = (index >= 0) & ~(best < 1e-4)
    return np.where(valid, index, -1), best, valid


def g2l64(points, frames, cfg, index):
    """(F, 4, 4) float64 = LOCAL_TO_LOCAL_SEARCH[index] @ [R^T | -R^T p]; 0 where index is -1."""
    tb = cfg.tables()
    L, T = cfg.shape
    dep, cs, sn = (tb[k].numpy().astype(np.float64) for k in ("depth", "cos", "sin"))
    out = np.zeros((len(points), 4, 4))
    for f, i in enumerate(index):
        if i < 0:
            continue
        R, p = np.asarray(frames[f], np.float64), np.asarray(points[f], np.float64)
        G = np.eye(4)
        G[:3, :3], G[:3, 3] = R.T, -(R.T @ p)
        S = np.eye(4)
        d, t = divmod(int(i), T)
        S[0, 3] = -dep[d]
        S[1, 1], S[1, 2], S[2, 1], S[2, 2] = cs[t], sn[t], -sn[t], cs[t]
        out[f] = S @ G
    return out


def bounds(gripper, x_range=None):
    x_lo, x_hi = (-gripper.bottom_length, gripper.finger_length) if x_range is None else x_range
    return _f32(x_lo), _f32(x_hi), _f32(gripper.half_bottom_space), _f32(gripper.half_hand_thickness)


def regions64(g2l, cloud, gripper, x_range=None, tol=TOL, sabotage=None):
    """g2l (F, 4, 4), cloud (3, N) -> list per frame of dict(certain, ambiguous: ascending index arrays; local: (3, N)
    float64 local coordinates with the y and z shifts).  A zero matrix gives empty sets."""
    x_lo, x_hi, hbs, hht = bounds(gripper, x_range)
    P = np.asarray(cloud, np.float64)
    out = []
    for G in np.asarray(g2l, np.float64):
        if not G.any():
            out.append(dict(certain=np.zeros(0, np.int64), ambiguous=np.zeros(0, np.int64), local=None))
            continue
        l = G[:3, :3] @ P + G[:3, 3:4]
        if sabotage == "face_ge":
            inside = (l[0] > x_lo) & (l[0] < x_hi) & (np.abs(l[1]) <= hbs) & (np.abs(l[2]) < hht)
        else:
            inside = (l[0] > x_lo) & (l[0] < x_hi) & (np.abs(l[1]) < hbs) & (np.abs(l[2]) < hht)
        wide = (l[0] > x_lo - tol) & (l[0] < x_hi + tol) & (np.abs(l[1]) < hbs + tol) & (np.abs(l[2]) < hht + tol)
        near = (np.abs(l[0] - x_lo) < tol) | (np.abs(l[0] - x_hi) < tol) | (np.abs(np.abs(l[1]) - hbs) < tol) | \
            (np.abs(np.abs(l[2]) - hht) < tol)
        amb = wide & near
        loc = l.copy()
        if sabotage != "no_y_shift":
            loc[1] += hbs
        loc[2] += hht
        out.append(dict(certain=np.nonzero(inside & ~amb)[0], ambiguous=np.nonzero(amb)[0], local=loc))
    return out


def units32(proj, gripper):
    return np.array(proj.units(gripper), np.float32)


def heights64(proj, gripper):
    """(3, R): torch.linspace(unit / 2, dim - unit / 2, R) per axis in float64 (:379-381); (k + 0.5) * unit for margin 0."""
    R = proj.resolution
    out = np.zeros((3, R))
    for a, d in enumerate(proj.dims(gripper)):
        u = d / (R - proj.margin)
        out[a] = 0.5 * u + np.arange(R) * ((d - u) / (R - 1))
    return out


def voxels32(points_f32, proj, gripper):
    """(3, n) int64 voxel indices by the exact fp32 rule, and which points fall inside the grid."""
    q = np.floor(np.asarray(points_f32, np.float32) / units32(proj, gripper)[:, None]).astype(np.int64)
    return q, ((q >= 0) & (q < proj.resolution)).all(0)


def projection64(points_f32, normals_f32, proj, gripper, sabotage=None):
    """points, normals (3, n) fp32 -> (12, R, R) float64, and the largest per-voxel count."""
    R = proj.resolution
    q, ok = voxels32(points_f32, proj, gripper)
    q, nr = q[:, ok], np.asarray(normals_f32, np.float64)[:, ok]
    cnt = np.zeros((R, R, R))
    sm = np.zeros((3, R, R, R))
    np.add.at(cnt, (q[0], q[1], q[2]), 1)
    for c in range(3):
        np.add.at(sm[c], (q[0], q[1], q[2]), nr[c])
    mean = sm if sabotage == "voxel_sum" else sm / np.maximum(cnt, 1)
    occ = cnt if sabotage == "occ_count" else (cnt > 0).astype(np.float64)
    H = heights64(proj, gripper)
    out = np.zeros((12, R, R))
    orders = ((0, 1, 2), (2, 1, 0), (2, 0, 1)) if sabotage == "order" else ORDERS
    for i, o in enumerate(orders):
        po = occ.transpose(o)
        pm = mean.transpose((0,) + tuple(a + 1 for a in o))
        n_occ = cnt.transpose(o).sum(2) if sabotage == "div_points" else po.sum(2)
        den = np.maximum(n_occ, 1e-4)
        h = H[o[0] if sabotage == "height_axis" else o[2]]
        out[4 * i] = (po * h).sum(2) / den
        out[4 * i + 1:4 * i + 4] = pm.sum(3) / den
    return out, int(cnt.max()) if cnt.size else 0


def map_bound(points_f32, normals_f32, proj, gripper):
    """(12, 1, 1) bound of the kernel's distance from `projection64` of the same fp32 set, derived, not measured:
    (m + 64) * 2^-24 * s, m = the largest per-voxel count (the voxel sum: m terms, each within 2^-31 of its fixed-point
    value and the sum exact), 64 covers the at most 60-term line sum in fp32 and the divisions, s = the largest |normal
    component| for the normal channels and the box dimension for the height channels."""
    _, m = projection64(points_f32, normals_f32, proj, gripper)
    q, ok = voxels32(points_f32, proj, gripper)
    s = float(np.abs(np.asarray(normals_f32, np.float64)[:, ok]).max()) if ok.any() else 0.0
    b = np.zeros((12, 1, 1))
    for i, o in enumerate(ORDERS):
        b[4 * i] = (m + 64) * 2.0 ** -24 * proj.dims(gripper)[o[2]]
        b[4 * i + 1:4 * i + 4] = (m + 64) * 2.0 ** -24 * s
    return b


def pixel_mask(local64, proj, gripper, vtol=VTOL):
    """(12, R, R) bool: the pixels a point of local64 (3, n) float64 within vtol of a voxel face (or of the grid's end)
    can move between, in every channel of the map they belong to."""
    R = proj.resolution
    u = units32(proj, gripper).astype(np.float64)[:, None]
    c = np.asarray(local64, np.float64) / u
    lo, hi = np.floor(c - vtol / u).astype(np.int64), np.floor(c + vtol / u).astype(np.int64)
    mask = np.zeros((12, R, R), bool)
    for j in np.nonzero((lo != hi).any(0))[0]:
        for vx in {lo[0, j], hi[0, j]}:
            for vy in {lo[1, j], hi[1, j]}:
                for vz in {lo[2, j], hi[2, j]}:
                    v = (vx, vy, vz)
                    for i, o in enumerate(ORDERS):
                        a, b = v[o[0]], v[o[1]]
                        if 0 <= a < R and 0 <= b < R:
                            mask[4 * i:4 * i + 4, a, b] = True
    return mask


def _ulps(v):
    f = np.float32(v)
    return float(f), float(np.nextafter(f, np.float32(np.inf))), float(np.nextafter(f, np.float32(-np.inf)))


def face_cloud(gripper, x_range=None):
    """For an IDENTITY matrix (every transform exact in fp32): one point exactly on every face of the region, one an ulp
    inside it and one an ulp outside it, and one in the middle.  -> (cloud (3, M) fp32, member (M,) bool)."""
    x_lo, x_hi, hbs, hht = bounds(gripper, x_range)
    xin = 0.03125
    assert x_lo < xin < x_hi
    pts, member = [(xin, 0.0, 0.0)], [True]
    for axis, face, inward in ((0, x_lo, 1), (0, x_hi, -1), (1, hbs, -1), (1, -hbs, 1), (2, hht, -1), (2, -hht, 1)):
        on, up, dn = _ulps(face)
        for v, m in ((on, False), (up, inward > 0), (dn, inward < 0)):
            p = [xin, 0.0, 0.0]
            p[axis] = v
            pts.append(tuple(p))
            member.append(m)
    return np.array(pts, np.float32).T.copy(), np.array(member)


def blob_frames(rng, n_points, n_frames, gripper, n_in=40):
    """A cloud of n_points (3, N) of which min(n_points, n_in) lie inside the close region of a base matrix and the rest
    30 cm away, unit-ish normals, and n_frames rigid matrices (F, 4, 4) near the base one (turned by up to 0.1 rad, moved
    by up to 3 mm): every frame's region holds points.  All fp32."""
    def rot(axis, ang):
        axis = axis / np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    base = rot(rng.standard_normal(3), rng.uniform(0, np.pi))
    origin = rng.uniform(-0.2, 0.2, 3) + np.array([0, 0, 1.0])
    k = min(n_points, n_in)
    loc = np.stack([rng.uniform(0.005, 0.08, k), rng.uniform(-0.025, 0.025, k), rng.uniform(-0.008, 0.008, k)], 1)
    far = rng.uniform(-0.05, 0.05, (n_points - k, 3)) + np.array([0.3, 0.3, 0.0])
    pts = np.concatenate([loc, far]) @ base.T + origin
    o = rng.permutation(n_points)
    nrm = rng.standard_normal((3, n_points))
    nrm /= np.linalg.norm(nrm, axis=0, keepdims=True)
    G = np.zeros((n_frames, 4, 4))
    for f in range(n_frames):
        Rm = (rot(rng.standard_normal(3), rng.uniform(0, 0.1)) @ base) if f else base
        p = origin + (rng.uniform(-0.003, 0.003, 3) if f else 0)
        G[f, :3, :3], G[f, :3, 3], G[f, 3, 3] = Rm.T, -(Rm.T @ p), 1
    return pts[o].T.astype(np.float32).copy(), nrm.astype(np.float32), G.astype(np.float32)
