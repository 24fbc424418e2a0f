"""Exact references for the batched frame grading (`postprocess.eval_frames`, csrc/eval_frames.hip; the reference's
`EvalExpCloud.eval_frame`, eval_experiment/eval_point_cloud.py:39-113).  TEST INFRASTRUCTURE ONLY; built on
tests/collision_ref.py, which stays as it is.

  * `grade64`         every integer and float of a pose in float64 (exact products of the fp32 inputs), plus per deciding
                      quantity the number of AMBIGUOUS points: closer than `tol` to a face or a band boundary that
                      decides it.  An fp32 implementation may differ from the float64 count by at most those.
  * `decided`         the poses whose flags no ambiguous point can turn.
  * `clearance_scene` poses and clouds built in each pose's local frame with every coordinate at least `delta` away
                      from every face and both band boundaries: all six integers hold by construction.
  * `face_scene`      signed-permutation poses (every transform exact): points exactly on, one ulp inside and one ulp
                      outside each deciding face and each band boundary.

The kernel's loop structure (what EDGE_SHAPES has to cross): chunks per scene = ceil(N / 8 192) within [8, 64] (so the
chunk count turns at N = 65 536 / 65 537 and stays 64 from N = 516 097; chunks are empty below N = 50 as in the
collision counter); sweeps of 1 024 points; 16 workgroups share a scene's poses; 32 poses per workgroup and pass, so
passes start at poses 512 and 1 024 (the second scan compacts the scored poses of a pass: a pass may hold none).
"""
import numpy as np
import torch

from tests import collision_ref as CR

SCORE_TOL = 1e-4        # the issue's bar: scores and means within 1e-4 of float64 (their scale is 1)

# collision_ref.EDGE_SHAPES plus: the chunk count's turn (65 536 -> 8 chunks of 8 192, 65 537 -> 9) and one scene of
# more than 400 000 points (50 chunks)
EDGE_SHAPES = list(CR.EDGE_SHAPES) + [(1, 65536, 33), (1, 65537, 16), (2, 409601, 50)]

INT_FIELDS = ("back", "finger", "close", "multi_objects", "n_left", "n_right")
FLOAT_FIELDS = ("left_y", "right_y", "mean_left", "mean_right", "score")


def params(gripper):
    fc = CR.faces(gripper)
    f = lambda v: float(np.float32(v))
    fc.update(back_thr=f(gripper.back_collision_threshold), fing_thr=f(gripper.finger_collision_threshold),
              min_points=f(gripper.close_region_min_points), nd=f(gripper.neighbor_depth))
    return fc


def grade64(g2l, cloud, normals, labels, gripper, tol=4e-6, chunk=16, sabotage=None, band_dtype=np.float64):
    """g2l (K, 4, 4) fp32 global -> local matrices, cloud / normals (3, N) fp32, labels (N,) int; numpy or torch
    (float64 work happens on the cloud's device).  -> dict of numpy arrays of length K: the INT_FIELDS, `collision`,
    `scored`, the FLOAT_FIELDS (float64) and the ambiguous counts `amb_back`, `amb_finger`, `amb_close` (points within
    `tol` of a face deciding that region), `amb_label` (True when ambiguous close-region points carry a label the
    certain ones do not -- or the certain ones hold none), `amb_left`, `amb_right` (close-region points within `tol` of
    the band's boundary).
    band_dtype=np.float32: the band bounds from fp32 arithmetic on the float64 extrema -- for scenes whose local
    coordinates are exact fp32 values (`face_scene`), where it makes every integer the exact fp32 answer.
    sabotage (the yardstick's own tests): "normals" leaves the normals unrotated, "band_x" tests x in place of y in the
    bands, "min_points_ge" gates with `close <= min_points` in place of `<`."""
    P = torch.as_tensor(cloud)
    dev = P.device
    G = torch.as_tensor(g2l).to(dev).double()
    p = P.double()
    nrm = torch.as_tensor(normals).to(dev).double()
    lab = torch.as_tensor(labels).to(dev).long()
    fc = params(gripper)
    K = G.shape[0]
    out = {k: np.zeros(K, np.int64) for k in INT_FIELDS + ("amb_back", "amb_finger", "amb_close", "amb_left", "amb_right")}
    out.update({k: np.zeros(K, np.float64) for k in FLOAT_FIELDS})
    out.update({k: np.zeros(K, bool) for k in ("collision", "scored", "amb_label")})
    near = lambda v, fs: torch.stack([(v - f).abs() for f in fs]).amin(dim=0) < tol
    inside = lambda v, lo, hi: (v > lo - tol) & (v < hi + tol)
    BIG = 2 ** 40
    for k0 in range(0, K, chunk):
        g = G[k0:k0 + chunk]
        loc = torch.matmul(g[:, :3, :3], p) + g[:, :3, 3:]                    # (k, 3, N)
        x, y, z = loc[:, 0], loc[:, 1], loc[:, 2]
        back, fing = CR._counts_local(x, y, z, fc)
        closer = (x < fc["fl"]) & (x > -fc["bl"]) & (z < fc["hht"]) & (z > -fc["hht"]) & (y < fc["hbs"]) & (y > -fc["hbs"])
        region = inside(x, -fc["bl"], fc["fl"]) & inside(z, -fc["hht"], fc["hht"]) & inside(y, -fc["hbw"], fc["hbw"])
        xz = near(x, [fc["fl"], -fc["bl"]]) | near(z, [fc["hht"], -fc["hht"]])
        amb_back = region & (xz | near(x, [-fc["m"]]) | near(y, [fc["hbw"], -fc["hbw"]]))
        amb_fing = region & (xz | near(y, [fc["hbw"], -fc["hbw"], fc["hbs"], -fc["hbs"]]))
        amb_close = region & inside(y, -fc["hbs"], fc["hbs"]) & (xz | near(y, [fc["hbs"], -fc["hbs"]]))
        sure = closer & ~amb_close
        l2 = lab.view(1, -1)
        lmin = torch.where(closer, l2, BIG).amin(1)
        lmax = torch.where(closer, l2, -BIG).amax(1)
        smin, smax = torch.where(sure, l2, BIG).amin(1), torch.where(sure, l2, -BIG).amax(1)
        amin, amax = torch.where(amb_close, l2, BIG).amin(1), torch.where(amb_close, l2, -BIG).amax(1)
        n_close = closer.sum(1)
        multi = (n_close > 0) & (lmin != lmax)
        # can the ambiguous points change the verdict?  only where the certain points do not already hold two labels
        have_amb = amb_close.any(1)
        amb_label = have_amb & ~(smin < smax) & ((sure.sum(1) == 0) | (amin != smin) | (amax != smax) | (amin != amax))
        left_y = torch.where(closer, y, -np.inf).amax(1)
        right_y = torch.where(closer, y, np.inf).amin(1)
        if band_dtype == np.float32:
            d = np.minimum((left_y.cpu().numpy().astype(np.float32) - right_y.cpu().numpy().astype(np.float32))
                           / np.float32(3), np.float32(fc["nd"]))
            lthr = torch.as_tensor((left_y.cpu().numpy().astype(np.float32) - d).astype(np.float64)).to(dev)
            rthr = torch.as_tensor((right_y.cpu().numpy().astype(np.float32) + d).astype(np.float64)).to(dev)
        else:
            d = torch.clamp((left_y - right_y) / 3, max=fc["nd"])
            lthr, rthr = left_y - d, right_y + d
        v = x if sabotage == "band_x" else y
        if sabotage == "band_x":
            lx, rx = torch.where(closer, x, -np.inf).amax(1), torch.where(closer, x, np.inf).amin(1)
            d = torch.clamp((lx - rx) / 3, max=fc["nd"])
            lthr, rthr = lx - d, rx + d
        il = closer & (v > lthr.view(-1, 1))
        ir = closer & (v < rthr.view(-1, 1))
        ny = nrm[1].view(1, -1).expand(len(g), -1) if sabotage == "normals" else torch.matmul(g[:, 1:2, :3], nrm)[:, 0]
        a = ny.abs()
        nl, nr = il.sum(1), ir.sum(1)
        ml = torch.where(il, a, 0.0).sum(1) / nl
        mr = torch.where(ir, a, 0.0).sum(1) / nr
        wide = region & inside(y, -fc["hbs"], fc["hbs"])
        amb_l = (wide & ((v - lthr.view(-1, 1)).abs() < tol)).sum(1)
        amb_r = (wide & ((v - rthr.view(-1, 1)).abs() < tol)).sum(1)
        nb, nf = back.sum(1), fing.sum(1)
        collision = (nb > fc["back_thr"]) | (nf > fc["fing_thr"])
        few = (n_close <= fc["min_points"]) if sabotage == "min_points_ge" else (n_close < fc["min_points"])
        scored = (n_close > 0) & ~few & ~collision & ~multi
        s = slice(k0, k0 + len(g))
        c = lambda t: t.cpu().numpy()
        out["back"][s], out["finger"][s], out["close"][s] = c(nb), c(nf), c(n_close)
        out["multi_objects"][s], out["collision"][s], out["scored"][s] = c(multi), c(collision), c(scored)
        out["amb_back"][s], out["amb_finger"][s], out["amb_close"][s] = c(amb_back.sum(1)), c(amb_fing.sum(1)), c(amb_close.sum(1))
        out["amb_label"][s], out["amb_left"][s], out["amb_right"][s] = c(amb_label), c(amb_l), c(amb_r)
        has = c(n_close > 0)
        out["left_y"][s] = np.where(has, c(left_y), 0.0)
        out["right_y"][s] = np.where(has, c(right_y), 0.0)
        sc = c(scored)
        out["n_left"][s], out["n_right"][s] = np.where(sc, c(nl), 0), np.where(sc, c(nr), 0)
        out["mean_left"][s], out["mean_right"][s] = np.where(sc, c(ml), 0.0), np.where(sc, c(mr), 0.0)
        out["score"][s] = np.where(sc, c(ml) * c(mr), 0.0)
    return out


def grade64_batch(g2l, cloud, normals, labels, gripper, **kw):
    """`grade64` per scene of a batch -> dict of (B, K) arrays."""
    rs = [grade64(g2l[b], cloud[b], normals[b], labels[b], gripper, **kw) for b in range(len(cloud))]
    return {k: np.stack([r[k] for r in rs]) for k in rs[0]}


def decided(r, gripper):
    """Boolean per pose: no threshold (back, finger, min points) lies within the ambiguous count of the float64 count
    and no ambiguous point carries the only second label -- every flag, and whether the pose is scored, is then the same
    for any implementation that differs from float64 on ambiguous points only."""
    fc = params(gripper)
    side = lambda n, a, thr: (n - a > thr) | (n + a <= thr)                  # verdict n > thr
    ok = side(r["back"], r["amb_back"], fc["back_thr"]) & side(r["finger"], r["amb_finger"], fc["fing_thr"])
    ok &= (r["close"] - r["amb_close"] >= fc["min_points"]) | (r["close"] + r["amb_close"] < fc["min_points"])
    return ok & ~r["amb_label"]


def outcome(collision, multi, score_nonzero):
    """The five outcome classes of a pose: 0 scored, 1 collision, 2 collision and multi-object, 3 multi-object only,
    4 too few points (no flag, no score)."""
    collision, multi, score_nonzero = map(np.asarray, (collision, multi, score_nonzero))
    return np.where(collision & multi, 2, np.where(collision, 1, np.where(multi, 3, np.where(score_nonzero, 0, 4))))


def noisy_normals(rng, n):
    v = rng.standard_normal((3, n))
    v /= np.linalg.norm(v, axis=0, keepdims=True)
    return (v * (1 + rng.uniform(-0.02, 0.02, n))).astype(np.float32)


def clearance_scene(rng, B, N, K, gripper, delta=1e-4):
    """-> (poses (B, K, 4, 4) fp32 gripper -> global, cloud (B, 3, N), normals (B, 3, N) fp32, labels (B, N) int32,
    expected: dict of (B, K) int64 arrays for INT_FIELDS).

    As `collision_ref.clearance_scene`: pose k sits at its own node of a grid, its points are drawn in its LOCAL frame
    cell by cell with every coordinate at least `delta` from every face, mapped to the global frame in float64 and
    rounded to fp32; the cloud is shuffled.  Here the cells are: behind the palm between the fingers (back AND close
    region), behind the palm in a finger (back and finger), in a finger, between the fingers (close region only),
    outside.  Per pose the close-region population is drawn around 50 (49, 50 and 51 among them), the back count
    around 10 sqrt(8), the finger count around 10, and one pose in four gets a second label on a few close-region
    points.  The close region's y values are laid out for prescribed bands: one point at the top y1 and one at the
    bottom y0 (the extrema), nl - 1 further points in (y1 - depth + delta, y1 - delta), nr - 1 in (y0 + delta,
    y0 + depth - delta), the rest in (y0 + depth + delta, y1 - depth - delta), with depth = min((y1 - y0) / 3, 0.005)
    (y1 - y0, between a tenth of and the whole gap so that both branches of the min occur, is kept away from
    3 x 0.005 by 10 delta): the fp32 extrema move by 1e-7, far less than delta, so both band
    populations hold by construction.  A pose takes all its points or none (when N runs out: the last pose and those
    at the edges of the kernel's 512-pose passes first); the rest of N is filled outside every box and, one in ten,
    inside pose 0's finger / back-and-finger cells."""
    fc = params(gripper)
    reach = 0.05
    cx, cy, cz = CR._cells(fc, reach)
    box = np.sqrt((fc["bl"] + reach) ** 2 + (fc["hbw"] + reach) ** 2 + (fc["hht"] + reach) ** 2)
    far = box + 0.05
    side = int(np.ceil(K ** (1 / 3)))
    spacing = 2 * far + 0.1
    X1 = [c for c in cx if c[1] <= -fc["m"] and c[0] >= -fc["bl"]][0]
    X2 = [c for c in cx if c[0] >= -fc["m"] and c[1] <= fc["fl"]][0]
    Y3, Z1 = cy[3], cz[1]
    hbs, nd = fc["hbs"], fc["nd"]

    def draw(cell, n):
        return CR._draw(rng, cell[0], cell[1], delta, n) if n else np.zeros(0)

    def outside(n):
        out = np.zeros((0, 3))
        while len(out) < n:
            m = 2 * (n - len(out)) + 8
            q = np.stack([CR._draw(rng, *np.array(c)[rng.integers(len(c), size=m)].T, delta, m) for c in (cx, cy, cz)], 1)
            inx = (q[:, 0] < fc["fl"]) & (q[:, 0] > -fc["bl"])
            inz = np.abs(q[:, 2]) < fc["hht"]
            out = np.concatenate([out, q[~(inx & inz & (np.abs(q[:, 1]) < fc["hbw"]))]])
        return out[:n]

    poses = np.zeros((B, K, 4, 4), np.float32)
    cloud = np.zeros((B, 3, N), np.float32)
    normals = np.zeros((B, 3, N), np.float32)
    labels = np.zeros((B, N), np.int32)
    exp = {k: np.zeros((B, K), np.int64) for k in INT_FIELDS}
    for b in range(B):
        R = CR._random_rotations(rng, K)
        node = np.stack(np.unravel_index(np.arange(K), (side, side, side)), 1) * spacing
        t = node - node.mean(0) + rng.uniform(-0.01, 0.01, (K, 3))
        poses[b, :, :3, :3], poses[b, :, :3, 3], poses[b, :, 3, 3] = R, t, 1
        Rf, tf = poses[b, :, :3, :3].astype(np.float64), poses[b, :, :3, 3].astype(np.float64)
        chunks, labs, used = [], [], 0
        edge = list(dict.fromkeys(k for k in (K - 1, 512, 1024, 511, 1023, 0) if k < K))
        rest = np.setdiff1d(np.arange(K), edge)
        for n_pose, k in enumerate(edge + list(rng.permutation(rest))):
            n_close = int((49, 50, 51)[n_pose % 3] if n_pose < 6 else rng.integers(40, 64))
            nb = int(rng.integers(0, 27) if rng.random() < 0.7 else rng.integers(27, 36))    # collides iff nb > 28
            nf = int(rng.integers(0, 10) if rng.random() < 0.7 else rng.integers(9, 15))     # collides iff nf > 10
            both = int(rng.integers(0, min(nb, nf) + 1))
            n_bc = nb - both                                  # behind the palm, between the fingers: back AND close
            n_close = max(n_close, n_bc, 2)
            # the close region's y layout
            y1 = rng.uniform(0.05 * hbs, hbs - 2 * delta)
            y0 = -rng.uniform(0.05 * hbs, hbs - 2 * delta)
            if abs((y1 - y0) - 3 * nd) < 10 * delta:
                y1 += 20 * delta if y1 + 22 * delta < hbs else -20 * delta
            depth = min((y1 - y0) / 3, nd)
            nl = int(rng.integers(1, max(2, n_close // 3)))
            nr = int(rng.integers(1, max(2, n_close // 3)))
            ys = np.concatenate([[y1], rng.uniform(y1 - depth + delta, y1 - delta, nl - 1),
                                 [y0], rng.uniform(y0 + delta, y0 + depth - delta, nr - 1),
                                 rng.uniform(y0 + depth + delta, y1 - depth - delta, n_close - nl - nr)])
            ys = ys[rng.permutation(n_close)]
            xs = np.concatenate([draw(X1, n_bc), draw(X2, n_close - n_bc)])
            close_pts = np.stack([xs, ys, draw(Z1, n_close)], 1)
            bf = np.stack([draw(X1, both), draw(Y3, both) * np.where(rng.random(both) < 0.5, 1, -1), draw(Z1, both)], 1)
            fo = np.stack([draw(X2, nf - both), draw(Y3, nf - both) * np.where(rng.random(nf - both) < 0.5, 1, -1),
                           draw(Z1, nf - both)], 1)
            loc = np.concatenate([close_pts, bf, fo, outside(int(rng.integers(8, 25)))])
            if used + len(loc) > N:
                continue                                       # all of a pose's points or none
            base = int(rng.integers(1, 1000))
            lb = rng.integers(1, 1000, len(loc))               # labels outside the close region do not matter
            lb[:n_close] = base
            two = rng.random() < 0.25
            if two:
                lb[rng.permutation(n_close)[:int(rng.integers(1, 4))]] = base + 1
            collision = nb > fc["back_thr"] or nf > fc["fing_thr"]
            scored = n_close >= fc["min_points"] and not collision and not two
            exp["back"][b, k], exp["finger"][b, k], exp["close"][b, k] = nb, nf, n_close
            exp["multi_objects"][b, k] = two
            exp["n_left"][b, k], exp["n_right"][b, k] = (nl, nr) if scored else (0, 0)
            chunks.append(np.einsum("ij,nj->ni", Rf[k], loc) + tf[k])
            labs.append(lb)
            used += len(loc)
        if used < N:
            n = N - used
            ks = rng.integers(0, K, n)
            inner = rng.random(n) < 0.1
            ks[inner] = 0
            loc = outside(n)
            for j in np.nonzero(inner)[0]:
                c = int(rng.integers(2))                      # 0: back and finger, 1: finger only
                loc[j] = (draw(X1 if c == 0 else X2, 1)[0], draw(Y3, 1)[0] * (1 if rng.random() < 0.5 else -1),
                          draw(Z1, 1)[0])
                exp["back"][b, 0] += c == 0
                exp["finger"][b, 0] += 1
            chunks.append(np.einsum("kij,kj->ki", Rf[ks], loc) + tf[ks])
            labs.append(rng.integers(1, 1000, n))
            if exp["back"][b, 0] > fc["back_thr"] or exp["finger"][b, 0] > fc["fing_thr"]:
                exp["n_left"][b, 0] = exp["n_right"][b, 0] = 0
        o = rng.permutation(N)
        cloud[b] = np.concatenate(chunks)[o].T.astype(np.float32)
        labels[b] = np.concatenate(labs)[o].astype(np.int32)
        normals[b] = noisy_normals(rng, N)
    return poses, cloud, normals, labels, exp


def edge_scene(B, N, K):
    """The clearance scene of an EDGE_SHAPES case, seeded by its shape: the non-default box except where
    (N + K) % 5 == 0."""
    gripper = CR.gripper_config(odd=(N + K) % 5 != 0)
    return (gripper,) + clearance_scene(np.random.default_rng(N * 11 + K), B, N, K, gripper)


def face_gripper(odd):
    """The box of the face scene: 4 points make a close region, NEIGHBOR_DEPTH = 2^-8 is an exact fp32 value, and the
    collision thresholds are out of reach (every pose sees every pose's points: hundreds in each region)."""
    from s4g_release_amd.postprocess import GripperConfig
    return GripperConfig(close_region_min_points=4, neighbor_depth=2.0 ** -8, back_collision_threshold=1e4,
                         finger_collision_threshold=1e4, **(CR.ODD_GRIPPER if odd else {}))


def face_scene(gripper):
    """-> (poses (1, 24, 4, 4), cloud (1, 3, M), normals (1, 3, M) fp32, labels (1, M) int32, expected: `grade64` of the
    scene with band_dtype=float32, as (1, 24) arrays).

    The 24 signed-permutation poses, zero translation: every local coordinate of every point under every pose is a
    coordinate of the cloud, exactly, so the float64 classification with fp32 band arithmetic IS the exact fp32 answer
    (the faces of the two collision regions alone: `collision_ref.face_scene`, compared with the collision counter).
    Per pose, in its local frame: points exactly on, one ulp inside and one ulp outside each face of the close region
    (finger_length, -bottom_length in x; +-half_hand_thickness in z; +-half_bottom_space in y, shared with the
    fingers), of which each pose takes a fixed random half, and ALWAYS the two points one ulp inside +-half_bottom_space:
    they are the extrema L and -L of the close region, depth = min(2 L / 3, 2^-8) = 2^-8, and both band bounds
    +-(L - 2^-8) are exact fp32 values (L and the bound differ by a multiple of L's ulp and the bound lies in L's binade
    or the one below).  Points exactly on each bound, one ulp inside and one ulp outside it.  One label everywhere and
    thresholds out of reach: no collision, so every pose is scored."""
    fc = params(gripper)
    f32 = np.float32
    up = lambda v: float(np.nextafter(f32(v), f32(np.inf)))
    dn = lambda v: float(np.nextafter(f32(v), f32(-np.inf)))
    three = lambda v: (float(f32(v)), up(v), dn(v))
    Rs = CR.signed_permutations()
    xf = float(f32(0.5 * (fc["fl"] - fc["m"])))
    yb = float(f32(0.25 * fc["hbs"]))
    L = dn(fc["hbs"])
    bound = L - 2.0 ** -8
    assert fc["nd"] == 2.0 ** -8 and 2 * L / 3 > 2.0 ** -8 and float(f32(bound)) == bound
    local = []
    for v in (fc["fl"], -fc["bl"]):
        local += [(w, yb, 0.0) for w in three(v)]
    for v in (fc["hht"], -fc["hht"]):
        local += [(xf, -yb, w) for w in three(v)]
    local += [(xf, w, 0.0) for w in (fc["hbs"], up(fc["hbs"]), -fc["hbs"], dn(-fc["hbs"]))]
    for v in (bound, -bound):
        local += [(xf, w, 0.0) for w in three(v)]
    must = [(xf, L, 0.0), (xf, -L, 0.0), (xf, 0.0, 0.0), (xf, yb / 2, 0.0)]
    local, must = np.array(local, np.float32), np.array(must, np.float32)
    keep = np.random.default_rng(11).random((len(Rs), len(local))) < 0.5
    cloud = np.concatenate([np.concatenate([must, local[keep[k]]]) @ R.T for k, R in enumerate(Rs)]).T.astype(np.float32)
    M = cloud.shape[1]
    normals = noisy_normals(np.random.default_rng(12), M)
    labels = np.full((1, M), 3, np.int32)
    poses = np.zeros((1, len(Rs), 4, 4), np.float32)
    poses[0, :, :3, :3] = Rs
    poses[0, :, 3, 3] = 1
    g2l = np.transpose(poses[0], (0, 2, 1)).copy()            # exact inverse: the transpose (zero translation)
    r = grade64(g2l, cloud, normals, labels[0], gripper, band_dtype=np.float32)
    return poses, np.ascontiguousarray(cloud[None]), normals[None], labels, {k: v[None] for k, v in r.items()}
