"""Exact references for the batched collision counter (`postprocess.view_non_collision`, csrc/pose_decode.hip
`collision_counts_kernel`; the reference's `CloudCollisionChecker.view_non_collision`,
cloud_processor/view_collision_checker.py:37-65).  TEST INFRASTRUCTURE ONLY.

The counter turns fp32 comparisons into integers, so it can be pinned exactly where no point lies within rounding of a
face that decides a counter:
  * `classify64`      the two counts per pose in float64, plus per counter the number of AMBIGUOUS points (closer than
                      `tol` to such a face): an fp32 implementation may differ from the float64 count by at most those;
  * `clearance_scene` random poses and clouds built in each pose's local frame with every coordinate at least `delta`
                      away from every face: the counts hold by construction, in any precision the transform keeps;
  * `face_scene`      signed-permutation poses (the 24 proper ones, zero translation), under which the fp32 transform
                      and both inverses are exact: points exactly ON each face and one fp32 ulp either side of it.
"""
import itertools

import numpy as np
import torch

BACK_THRESHOLD = 10 * np.sqrt(8)       # GripperConfig.back_collision_threshold
FINGER_THRESHOLD = 10


# a box that is not the default one: every parameter differs from its default, the margin is not zero
ODD_GRIPPER = dict(half_bottom_width=0.05, bottom_length=0.13, finger_width=0.019, half_hand_thickness=0.015,
                   finger_length=0.075, back_collision_margin=0.011)

# (B, N, K) where the kernel's loop structure turns (8 point chunks per scene, empty below N = 50; sweeps of 1 024
# points; 16 workgroups sharing a scene's poses; 32 poses per workgroup and pass, so passes start at poses 512 and
# 1 024): every N of {1, 2, 7, 8, 9, 14, 17, 33, 41, 43, 49, 50, 255, 1023, 1024, 1025, 8191, 8192, 8193, 24581, 48902}
# and every K of {1, 15, 16, 17, 32, 511, 512, 513, 1100}, crossed (not the full product)
EDGE_SHAPES = [(1, 1, 1), (3, 2, 17), (1, 7, 1100), (3, 8, 16), (1, 9, 15), (3, 14, 32), (1, 17, 513), (3, 33, 511),
               (3, 41, 1), (1, 43, 17), (3, 49, 512), (3, 50, 1100), (1, 255, 32), (3, 1023, 513), (1, 1024, 16),
               (1, 1025, 511), (1, 8191, 1100), (3, 8192, 15), (1, 8193, 512), (3, 24581, 1), (3, 48902, 1100),
               (1, 48902, 17)]
POSES_PER_PASS = 512


def gripper_config(odd):
    """`postprocess.GripperConfig`: the default box, or ODD_GRIPPER."""
    from s4g_release_amd.postprocess import GripperConfig
    return GripperConfig(**ODD_GRIPPER) if odd else GripperConfig()


def edge_scene(B, N, K):
    """The clearance scene of an EDGE_SHAPES case, seeded by its shape -> (gripper, poses, cloud, expected): the
    non-default box except where (N + K) % 5 == 0."""
    gripper = gripper_config(odd=(N + K) % 5 != 0)
    return (gripper,) + clearance_scene(np.random.default_rng(N * 7 + K), B, N, K, gripper)


def global2local(poses, inverse):
    """(..., 4, 4) fp32 poses -> the fp32 matrices the kernel applies: "se3" the analytic SE(3) inverse as the
    detector forms it (oracle `se3_inverse_f32`), "general" the float64 inverse rounded to fp32."""
    from oracle import postprocess as OP
    if inverse == "se3":
        return OP.se3_inverse_f32(poses.reshape(-1, 4, 4)).reshape(poses.shape)
    return np.linalg.inv(poses.astype(np.float64)).astype(np.float32)


def oracle_counts(poses, cloud, gripper, inverse):
    """The oracle's restatement of the reference's `view_non_collision` (oracle/postprocess.py) with `gripper`'s box
    and the given inverse -> (ok (B, K), counts (B, K, 2))."""
    from oracle import postprocess as OP
    return OP.view_non_collision(poses, cloud, half_bottom_width=gripper.half_bottom_width,
                                 bottom_length=gripper.bottom_length, finger_width=gripper.finger_width,
                                 half_hand_thickness=gripper.half_hand_thickness, finger_length=gripper.finger_length,
                                 back_margin=gripper.back_collision_margin,
                                 global2local=global2local(poses, "se3") if inverse == "se3" else None)


def faces(gripper):
    """The box of `gripper` (a `postprocess.GripperConfig`) as the kernel receives it: every face value rounded to fp32
    (the launcher passes `gripper6` as floats; the oracle compares fp32 coordinates against Python floats, in fp32)."""
    f = lambda v: float(np.float32(v))
    return dict(fl=f(gripper.finger_length), bl=f(gripper.bottom_length), hht=f(gripper.half_hand_thickness),
                hbw=f(gripper.half_bottom_width), hbs=f(gripper.half_bottom_space), m=f(gripper.back_collision_margin))


def verdicts(counts, gripper):
    """ok = back <= threshold and fingers <= threshold (`view_non_collision`)."""
    counts = np.asarray(counts)
    return (counts[..., 0] <= gripper.back_collision_threshold) & (counts[..., 1] <= gripper.finger_collision_threshold)


def _counts_local(x, y, z, fc):
    """Back / finger membership of local coordinates (view_collision_checker.py:39-60), any float dtype."""
    close = (x < fc["fl"]) & (x > -fc["bl"])
    zin = (z < fc["hht"]) & (z > -fc["hht"])
    back = close & zin & (y < fc["hbw"]) & (y > -fc["hbw"]) & (x < -fc["m"])
    fing = close & zin & (((y < fc["hbw"]) & (y > fc["hbs"])) | ((y > -fc["hbw"]) & (y < -fc["hbs"])))
    return back, fing


def classify64(g2l, cloud, gripper, tol=4e-6, chunk=32):
    """g2l (K, 4, 4) or (B, K, 4, 4) fp32 global -> local matrices (the inverse the kernel applies), cloud (3, N) or
    (B, 3, N) fp32, numpy or torch (float64 work happens on the tensors' device).  Returns numpy int64
    (counts (..., K, 2), ambiguous (..., K, 2)): counts classified in float64 (exact products of the fp32 inputs,
    one rounding per sum), ambiguous = points of the counter's region (widened by `tol`) within `tol` of a face that
    decides the counter -- back: x in {fl, -bl, -margin}, y in {+-hbw}, z in {+-hht}; fingers: x in {fl, -bl},
    y in {+-hbw, +-hbs}, z in {+-hht}."""
    G = torch.as_tensor(g2l)
    P = torch.as_tensor(cloud)
    single = P.dim() == 2
    if single:
        G, P = G.unsqueeze(0), P.unsqueeze(0)
    fc = faces(gripper)
    B, K = G.shape[:2]
    counts = torch.zeros((B, K, 2), dtype=torch.int64)
    amb = torch.zeros((B, K, 2), dtype=torch.int64)

    def near(v, fs):
        d = torch.stack([(v - f).abs() for f in fs]).amin(dim=0)
        return d < tol

    def inside(v, lo, hi):
        return (v > lo - tol) & (v < hi + tol)

    for b in range(B):
        p = P[b].double()
        for k0 in range(0, K, chunk):
            g = G[b, k0:k0 + chunk].to(p.device).double()
            loc = torch.matmul(g[:, :3, :3], p) + g[:, :3, 3:]                     # (k, 3, N) float64
            x, y, z = loc[:, 0], loc[:, 1], loc[:, 2]
            back, fing = _counts_local(x, y, z, fc)
            region = (inside(x, -fc["bl"], fc["fl"]) & inside(z, -fc["hht"], fc["hht"]) &
                      inside(y, -fc["hbw"], fc["hbw"]))
            zf = near(z, [fc["hht"], -fc["hht"]])
            amb_back = region & (near(x, [fc["fl"], -fc["bl"], -fc["m"]]) | near(y, [fc["hbw"], -fc["hbw"]]) | zf)
            amb_fing = region & (near(x, [fc["fl"], -fc["bl"]]) |
                                 near(y, [fc["hbw"], -fc["hbw"], fc["hbs"], -fc["hbs"]]) | zf)
            counts[b, k0:k0 + chunk] = torch.stack([back.sum(1), fing.sum(1)], 1).cpu()
            amb[b, k0:k0 + chunk] = torch.stack([amb_back.sum(1), amb_fing.sum(1)], 1).cpu()
    counts, amb = counts.numpy(), amb.numpy()
    return (counts[0], amb[0]) if single else (counts, amb)


def _random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def _cells(fc, reach):
    """Per axis, the open intervals between consecutive decisive faces (plus `reach` beyond the outermost ones)."""
    xs = sorted({-fc["bl"], -fc["m"], fc["fl"]})
    ys = [-fc["hbw"], -fc["hbs"], fc["hbs"], fc["hbw"]]
    zs = [-fc["hht"], fc["hht"]]
    mk = lambda fs: [(fs[0] - reach, fs[0])] + list(zip(fs[:-1], fs[1:])) + [(fs[-1], fs[-1] + reach)]
    return mk(xs), mk(ys), mk(zs)


def _draw(rng, lo, hi, delta, n):
    """n values in the open cells (lo, hi) (scalars or (n,) arrays), each at least delta from both ends: half uniform
    over the cell, half within 1 mm of one of its ends (clearance still >= delta)."""
    lo, hi = np.broadcast_to(lo, (n,)) + delta, np.broadcast_to(hi, (n,)) - delta
    assert (hi > lo).all()
    u = rng.uniform(lo, hi)
    edge = np.where(rng.random(n) < 0.5, lo + rng.uniform(0, 1e-3, n), hi - rng.uniform(0, 1e-3, n))
    return np.where(rng.random(n) < 0.5, u, np.clip(edge, lo, hi))


def clearance_scene(rng, B, N, K, gripper, delta=1e-4):
    """-> (poses (B, K, 4, 4) fp32 gripper -> global, cloud (B, 3, N) fp32, expected counts (B, K, 2) int64).

    Pose k of a scene sits at its own node of a 3-D grid (random proper rotation, the translation jittered), spaced so
    that no point drawn around one pose comes near another pose's box.  Around each pose, points are drawn in its LOCAL
    frame cell by cell (`_cells`: behind the palm, the two fingers, the gap, just outside each face, far): every local
    coordinate keeps `delta` from every face.  Per pose the back count is drawn around 10 sqrt(8) and the finger count
    around 10, so that verdicts fall on both sides of both thresholds.  Points are mapped to the global frame in
    float64 through the fp32 pose and rounded to fp32; the cloud's point order is shuffled (a pose's points spread over
    every chunk of the kernel).  Poses take their points until N is used up (the last pose and the poses at the edges of
    the kernel's 512-pose passes first, then the others in random order; the rest get none); a larger N is filled
    with points outside every box and, one in ten, inside pose 0's boxes (counts in the thousands)."""
    fc = faces(gripper)
    reach = 0.05
    cx, cy, cz = _cells(fc, reach)
    # local coordinates stay within `far` of the pose's origin; nodes 2 far + 0.1 apart
    box = np.sqrt((fc["bl"] + reach) ** 2 + (fc["hbw"] + reach) ** 2 + (fc["hht"] + reach) ** 2)
    far = box + 0.05
    side = int(np.ceil(K ** (1 / 3)))
    spacing = 2 * far + 0.1
    X1 = [c for c in cx if c[1] <= -fc["m"] and c[0] >= -fc["bl"]][0]          # behind the palm, in front of -bl
    X2 = [c for c in cx if c[0] >= -fc["m"] and c[1] <= fc["fl"]][0]           # between -margin and the finger tips
    Y1, Y2, Y3, Z1 = cy[1], cy[2], cy[3], cz[1]

    def pts(cells, n):
        return np.stack([_draw(rng, c[0], c[1], delta, n) for c in cells], 1) if n else np.zeros((0, 3))

    def outside(n):
        """n points of the pose's neighbourhood outside both counters' regions: one to three coordinates in an outer
        cell, or (one in five) far out, at a radius in [box, far)."""
        out = np.zeros((0, 3))
        while len(out) < n:
            m = 2 * (n - len(out)) + 8
            p = np.stack([_draw(rng, *np.array(c)[rng.integers(len(c), size=m)].T, delta, m) for c in (cx, cy, cz)], 1)
            back, fing = _counts_local(p[:, 0], p[:, 1], p[:, 2], fc)
            v = rng.standard_normal((m, 3))
            v *= (rng.uniform(box + 1e-3, far - 1e-3, m) / np.linalg.norm(v, axis=1))[:, None]
            far_out = rng.random(m) < 0.2
            p = np.where(far_out[:, None], v, p)
            out = np.concatenate([out, p[far_out | ~(back | fing)]])
        return out[:n]

    poses = np.zeros((B, K, 4, 4), np.float32)
    cloud = np.zeros((B, 3, N), np.float32)
    expected = np.zeros((B, K, 2), np.int64)
    for b in range(B):
        R = _random_rotations(rng, K)
        node = np.stack(np.unravel_index(np.arange(K), (side, side, side)), 1) * spacing
        t = node - node.mean(0) + rng.uniform(-0.01, 0.01, (K, 3))
        poses[b, :, :3, :3] = R
        poses[b, :, :3, 3] = t
        poses[b, :, 3, 3] = 1
        Rf, tf = poses[b, :, :3, :3].astype(np.float64), poses[b, :, :3, 3].astype(np.float64)
        chunks, used = [], 0
        # the order in which poses take points: the last pose and the first / last pose of every pass of the kernel's
        # pose loop first (32 slots x 16 workgroups = 512 poses per pass), then the others at random -- so that every
        # pass, the last partial one included, has points of its own even where N runs out after a few poses
        edge = list(dict.fromkeys(k for k in (K - 1, 512, 1024, 511, 1023, 0) if k < K))
        rest = np.setdiff1d(np.arange(K), edge)
        for k in edge + list(rng.permutation(rest)):
            if used >= N:
                break
            nb = int(rng.integers(22, 36))          # back threshold 28.28: ok iff nb <= 28
            nf = int(rng.integers(5, 16))           # finger threshold 10: ok iff nf <= 10
            both = int(rng.integers(0, min(nb, nf) + 1))
            fy = lambda n: np.where(rng.random(n) < 0.5, 1, -1)
            back_only = pts((X1, Y2, Z1), nb - both)
            back_fing = pts((X1, Y3, Z1), both)
            back_fing[:, 1] *= fy(both)
            fing_only = pts((X2, Y3, Z1), nf - both)
            fing_only[:, 1] *= fy(nf - both)
            gap = pts((X2, Y2, Z1), int(rng.integers(0, 8)))
            loc = np.concatenate([back_only, back_fing, fing_only, gap, outside(int(rng.integers(8, 25)))])
            tag = np.concatenate([np.full(nb - both, 1), np.full(both, 3), np.full(nf - both, 2),
                                  np.zeros(len(loc) - nb - (nf - both), int)])
            o = rng.permutation(len(loc))[:N - used]                 # (a partial pose when N runs out)
            loc, tag = loc[o], tag[o]
            expected[b, k] = ((tag & 1).astype(bool).sum(), (tag & 2).astype(bool).sum())
            chunks.append(np.einsum("ij,nj->ni", Rf[k], loc) + tf[k])
            used += len(loc)
        if used < N:                                                 # fill: outside every box, or inside pose 0's
            n = N - used
            ks = rng.integers(0, K, n)
            inner = rng.random(n) < 0.1
            ks[inner] = 0
            loc = outside(n)
            cells = [(X1, Y2, Z1), (X1, Y3, Z1), (X2, Y3, Z1)]
            for j in np.nonzero(inner)[0]:
                c = int(rng.integers(3))
                loc[j] = pts(cells[c], 1)[0]
                expected[b, 0] += (c != 2, c != 0)
            chunks.append(np.einsum("kij,kj->ki", Rf[ks], loc) + tf[ks])
        g = np.concatenate(chunks)[rng.permutation(N)]
        cloud[b] = g.T.astype(np.float32)
    return poses, cloud, expected


def signed_permutations():
    """The 24 proper rotations whose entries are 0 / +-1 (the rotation group of the cube), (24, 3, 3) fp32."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3), np.float32)
            R[range(3), perm] = signs
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    return np.stack(out)


def face_scene(gripper):
    """-> (poses (1, 24, 4, 4) fp32, cloud (1, 3, M) fp32, expected counts (1, 24, 2) int64).

    Poses: the 24 signed permutation rotations, zero translation -- every product in the fp32 transform is +-x or 0 and
    both the general inverse (float64, rounded) and the SE(3) inverse are exact transposes, so every local coordinate
    equals a coordinate of the cloud exactly, with or without FMA contraction.  For pose k, points are built in its
    local frame: one coordinate exactly on a decisive face (= float32(face value)), one fp32 ulp inside and one outside,
    the other two well inside the region that face decides (each pose takes a fixed random half of that list).
    Faces: finger_length and -bottom_length in x; +-half_hand_thickness in z; +-half_bottom_width and
    +-half_bottom_space in y; -back_collision_margin in x when the margin is not zero (with a zero margin the face
    is x = 0, whose ulp neighbours are fp32 denormals).  Every pose sees every pose's points (one cloud); the
    expected counts are those of exact fp32 comparisons: on-face points never count."""
    fc = faces(gripper)
    f32 = np.float32
    up = lambda v: float(np.nextafter(f32(v), f32(np.inf)))
    dn = lambda v: float(np.nextafter(f32(v), f32(-np.inf)))
    xb = float(f32(-0.5 * (fc["bl"] + fc["m"])))                    # behind the palm
    xf = float(f32(0.5 * (fc["fl"] - fc["m"])))                     # between the fingers' roots and tips
    yb = float(f32(0.5 * fc["hbs"]))                                # inside the palm's width, between the fingers
    yf = float(f32(0.5 * (fc["hbs"] + fc["hbw"])))                  # inside the right-side finger (+y)
    local = []
    for v in (fc["fl"], -fc["bl"]):                                 # x faces; y in the finger / the palm
        for y in (yf, -yf, yb):
            local += [(w, y, 0.0) for w in (v, up(v), dn(v))]
    if fc["m"] != 0:
        for y in (yb, yf):
            local += [(w, y, 0.0) for w in (-fc["m"], up(-fc["m"]), dn(-fc["m"]))]
    for v in (fc["hht"], -fc["hht"]):                               # z faces
        for x, y in ((xb, yb), (xb, yf), (xf, -yf)):
            local += [(x, y, w) for w in (v, up(v), dn(v))]
    for v in (fc["hbw"], -fc["hbw"], fc["hbs"], -fc["hbs"]):        # y faces
        for x in (xb, xf):
            local += [(x, w, 0.0) for w in (v, up(v), dn(v))]
    local = np.array(local, np.float32)
    Rs = signed_permutations()
    K = len(Rs)
    poses = np.zeros((1, K, 4, 4), np.float32)
    poses[0, :, :3, :3] = Rs
    poses[0, :, 3, 3] = 1
    # pose k contributes a fixed random half of the points (so that the counts differ from pose to pose: the whole
    # orbit under the group would give every pose the same counts, whatever rotation the kernel applied)
    keep = np.random.default_rng(7).random((K, len(local))) < 0.5
    cloud = np.concatenate([local[keep[k]] @ R.T for k, R in enumerate(Rs)]).T[None].astype(np.float32)   # p = R l
    # every local coordinate under every pose is an exact fp32 value: its fp32 comparisons are exact comparisons
    loc = np.einsum("kji,jn->kin", Rs.astype(np.float64), cloud[0].astype(np.float64))   # R^T p
    back, fing = _counts_local(loc[:, 0], loc[:, 1], loc[:, 2], fc)
    expected = np.stack([back.sum(1), fing.sum(1)], 1)[None].astype(np.int64)
    return poses, np.ascontiguousarray(cloud), expected
