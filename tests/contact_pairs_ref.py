"""Float64 yardstick of the contact model's per-object data: `GenerateContactObjectData`
(data_gen/data_generator/data_object_contact_point_generator.py) restated in numpy, all four stages -- the antipodal
pair search (`pairs`, :103-123), the per-pair grading over the rolled frames with the last-shift quirk (`grade`,
:125-221), the frames that come out (`frames`, :218) and the nearest object point of each (`nearest`, :79-86).  Every
stage returns its margins, so that a caller can tell the rows the reference's fp32 arithmetic decides from the rows it
does not.

Bounds are the reference's: formed in Python floats and rounded to fp32 once (torch compares an fp32 tensor with a
Python scalar in fp32), then used as exact float64 values.  Coordinates are float64 throughout, and the roll matrices
are the exact float64 inverses, not the fp32 `torch.inverse` of the reference: what fp32 does to both is what the
margin `eps` is there for.

THE DECIDED RULE.  A pair of the list is decided when its distance and its score lie further than PAIR_MARGIN from
their thresholds.  A (pair, roll) row is decided at eps when every count that a gate reads gives that gate the same
answer whether every bound is moved by +eps or by -eps (each strict inequality relaxed / tightened), and every close
count that enters the score is the same integer under both.  This is the interval form of "re-count with the bounds
moved by +-eps": the true fp32 count of a region lies between the two re-counts whichever way its points err, which
the two joint re-counts alone do not guarantee (a point may leave the palm region while another enters the close
region).  A row is exact when all nine counts of its roll and the pair's close-plane count are the same integers under
both.  eps is per pair: EPS0 / |x|, |x| the length of the un-normalised x axis (the conditioning of the frame).

SABOTAGES lists the mistakes tests/test_contact_pairs_ref.py plants; each names the stage it breaks."""
import numpy as np

HALF_BOTTOM_WIDTH, FINGER_WIDTH, HALF_HAND_THICKNESS = 0.057, 0.023, 0.012
FINGER_LENGTH, BOTTOM_LENGTH, BACK_COLLISION_MARGIN = 0.09, 0.08, 0.0
HALF_BOTTOM_SPACE = HALF_BOTTOM_WIDTH - FINGER_WIDTH
GASKET_RADIUS, COS_THR = 0.012, 0.95
THETA_SEARCH = tuple(range(0, 360, 30))
WIDTH_SHIFT = (-0.015, 0.015, 0)
MIN_POINTS, BACK_THRESHOLD, FINGER_THRESHOLD = 50, 0.0, 0
# float64 rounding of either form of the distance (sklearn's |x|^2 - 2 x.y + |y|^2 or the difference's norm) is below
# 1e-15 for points within a metre of the origin, that of the score below 1e-15 as well; 1e-9 is far above both and
# still leaves all but a handful of 14 M candidate pairs decided
PAIR_MARGIN = 1e-9
# squared distances of the nearest-point search: the centre comes out of fp32 products of entries below 1 with
# offsets below 0.5 m (error below 4 * 2^-24 * 0.5 = 1.2e-7 per coordinate, on either side: the reference inverts
# fp32 frames), and d < 0.2 m, so d^2 moves by less than 2 * 0.2 * 2 * 1.2e-7 = 1e-7; fp32 rounding of d^2 itself adds
# 3 * 2^-24 * 0.04 = 7e-9
NEAREST_MARGIN = 2e-7

SABOTAGES = ("no_triu", "one_sided_cos", "no_clip", "threshold_le", "dw_order", "max_dw", "no_third", "no_min",
             "rolls_reversed", "no_move_back", "back_without_close", "nearest_from_midpoint")


def f32(v):
    """A bound as the reference compares it: the Python float rounded to fp32 once, as a float64."""
    return float(np.float32(v))


def local_search_to_local(theta=THETA_SEARCH, move_back=True):
    """:29-37 in float64 -> (T, 4, 4)."""
    back = np.eye(4)
    if move_back:
        back[0, 3] = -(FINGER_LENGTH - GASKET_RADIUS)
    m = np.tile(np.eye(4), (len(theta), 1, 1))
    for i, th in enumerate(theta):
        m[i, 0, 0] = np.cos(th / 180 * np.pi)
        m[i, 2, 2] = np.cos(th / 180 * np.pi)
        m[i, 0, 2] = np.sin(th / 180 * np.pi)
        m[i, 2, 0] = -np.sin(th / 180 * np.pi)
    return m @ back


def local_to_local_search(theta=THETA_SEARCH, sabotage=None):
    theta = tuple(reversed(theta)) if sabotage == "rolls_reversed" else tuple(theta)
    return np.linalg.inv(local_search_to_local(theta, move_back=sabotage != "no_move_back"))


def pairs(points, normals, sabotage=None, max_distance=HALF_BOTTOM_SPACE * 2, cos_threshold=COS_THR, block=256):
    """points, normals (N, 3) -> dict: `row`, `col` (K,) in the order of np.nonzero(np.triu(...)), `score` (K,) float64,
    `decided` (K,) bool, and `near` (2, L): the (i, j), i < j, that are NOT in the list but within PAIR_MARGIN of both
    thresholds' wrong side (a device list may hold them)."""
    P, Nn = np.asarray(points, np.float64), np.asarray(normals, np.float64)
    N = len(P)
    rows, cols, scores, decided, near = [], [], [], [], []
    for i0 in range(0, N, block):
        i1 = min(N, i0 + block)
        dv = -P[i0:i1, None, :] + P[None, :, :]                       # [i, j] = p_j - p_i
        dist = np.sqrt(dv[..., 0] ** 2 + dv[..., 1] ** 2 + dv[..., 2] ** 2)
        with np.errstate(invalid="ignore", divide="ignore"):
            u = dv / (dist[..., None] if sabotage == "no_clip" else np.clip(dist[..., None], 0.0001, 1))
            cij = (u * Nn[i0:i1, None, :]).sum(-1)                    # u_ij . n_i
            cji = -(u * Nn[None, :, :]).sum(-1)                       # u_ji . n_j = -u_ij . n_j
            score = np.abs(cij) if sabotage == "one_sided_cos" else np.abs(cij * cji)
            keep = (dist < max_distance) & (score > cos_threshold)
        upper = np.arange(N)[None, :] > np.arange(i0, i1)[:, None]
        if sabotage != "no_triu":
            keep &= upper
        else:
            keep &= np.arange(N)[None, :] != np.arange(i0, i1)[:, None]
        with np.errstate(invalid="ignore"):
            close = (np.abs(dist - max_distance) <= PAIR_MARGIN) | (np.abs(score - cos_threshold) <= PAIR_MARGIN)
        r, c = np.nonzero(keep)
        rows.append(r + i0); cols.append(c); scores.append(score[r, c]); decided.append(~close[r, c])
        nr, nc = np.nonzero(close & ~keep & upper & (dist < max_distance + PAIR_MARGIN) &
                            (score > cos_threshold - PAIR_MARGIN))
        near.append(np.stack([nr + i0, nc]))
    return {"row": np.concatenate(rows), "col": np.concatenate(cols), "score": np.concatenate(scores),
            "decided": np.concatenate(decided), "near": np.concatenate(near, 1)}


def pair_frames(points, row, col):
    """:137-152 in float64 -> (T (K, 4, 4) global -> local, the rigid inverse; xlen (K,) the un-normalised |x|)."""
    P = np.asarray(points, np.float64)
    v = P[col] - P[row]
    with np.errstate(invalid="ignore", divide="ignore"):
        y = v / np.linalg.norm(v, axis=1, keepdims=True)
        x = np.array([[0.0, 1.0, 0.0]]) - y[:, 1:2] * y
        xlen = np.linalg.norm(x, axis=1)
        x = x / xlen[:, None]
    z = np.cross(x, y)
    R = np.stack([x, y, z], 2)                                        # columns
    c = (P[row] + P[col]) / 2
    T = np.zeros((len(row), 4, 4))
    T[:, :3, :3] = R.transpose(0, 2, 1)
    T[:, :3, 3] = -np.einsum("kji,kj->ki", R, c)
    T[:, 3, 3] = 1
    return T, xlen


def _gate(count_lo, count_hi, test):
    """(the gate's answer at the nominal count is between; True where lo and hi agree) for an integer test."""
    return test(count_lo) == test(count_hi)


def grade(points, row, col, eps0=0.0, sabotage=None, theta=THETA_SEARCH, shifts=WIDTH_SHIFT, min_points=MIN_POINTS,
          back_threshold=BACK_THRESHOLD, finger_threshold=FINGER_THRESHOLD):
    """points (N, 3), pair lists row, col (K,) -> dict over the K pairs and T rolls: `counts` (K, T, W, 3) = {back,
    finger, close}, `close_plane` (K,), `score` (K, T) float32, `valid` (K, T), `finite` (K,), `xlen` (K,), `T` (K, 4,
    4), and at eps = eps0 / xlen per pair: `decided` (K, T), `exact` (K, T)."""
    P = np.asarray(points, np.float64)
    K, nT, W = len(row), len(theta), len(shifts)
    L = local_to_local_search(theta, sabotage)
    order = list(range(W))
    if sabotage == "dw_order":
        order = order[::-1]
    hbs, hbw, hht = f32(HALF_BOTTOM_SPACE), f32(HALF_BOTTOM_WIDTH), HALF_HAND_THICKNESS
    margin, nbl, fl = f32(BACK_COLLISION_MARGIN), f32(-BOTTOM_LENGTH), f32(FINGER_LENGTH)
    zlo = np.array([f32(-hht + float(d)) for d in shifts])
    zhi = np.array([f32(hht + float(d)) for d in shifts])
    Tm, xlen = pair_frames(P, row, col)
    finite = np.isfinite(Tm).all((1, 2))
    counts = np.zeros((K, nT, W, 3), np.int64)
    plane = np.zeros(K, np.int64)
    score = np.zeros((K, nT), np.float32)
    valid = np.zeros((K, nT), bool)
    decided = np.zeros((K, nT), bool)
    exact = np.zeros((K, nT), bool)
    for k in range(K):
        if not finite[k]:
            continue
        eps = eps0 / xlen[k]
        local = Tm[k, :3, :3] @ P.T + Tm[k, :3, 3:]
        ay = np.abs(local[1])
        near = ay < hbw + eps
        local, ay = local[:, near], ay[near]
        s = L[:, :3, :3] @ local + L[:, :3, 3:]                       # (T, 3, n)
        sx, sz = s[:, 0], s[:, 2]
        got = {}
        for sign in (-1, 0, 1):
            e = sign * eps
            closep = ay < hbs + e
            fingp = (ay > hbs - e) & (ay < hbw + e)
            backp = fingp if sabotage == "back_without_close" else (fingp | closep)
            backx = (sx < margin + e) & (sx > nbl - e)
            fingx = (sx > margin - e) & (sx < fl + e)
            zin = (sz[:, None, :] < zhi[None, :, None] + e) & (sz[:, None, :] > zlo[None, :, None] - e)   # (T, W, n)
            c = np.stack([(backx[:, None] & zin & backp).sum(-1), (fingx[:, None] & zin & fingp).sum(-1),
                          (fingx[:, None] & zin & closep).sum(-1)], -1)
            got[sign] = (c, int(closep.sum()))
        counts[k], plane[k] = got[0]
        lo, hi = got[-1], got[1]
        plane_ok = plane[k] >= min_points
        plane_decided = (lo[1] >= min_points) == (hi[1] >= min_points)
        gt = (lambda a, b: a >= b) if sabotage == "threshold_le" else (lambda a, b: a > b)
        for t in range(nT):
            acc, last, biggest = np.float32(0), np.float32(0), np.float32(0)
            sure = plane_decided
            for w in order:
                b, f, c = (int(v) for v in counts[k, t, w])
                last = np.float32(0)
                sure = sure and _gate(lo[0][t, w, 0], hi[0][t, w, 0], lambda v: gt(v, back_threshold))
                if gt(b, back_threshold):
                    continue
                sure = sure and _gate(lo[0][t, w, 1], hi[0][t, w, 1], lambda v: gt(v, finger_threshold))
                if gt(f, finger_threshold):
                    continue
                last = np.float32(c)
                biggest = max(biggest, last)
                sure = sure and lo[0][t, w, 2] == hi[0][t, w, 2]
                if last < min_points:
                    continue
                acc = np.float32(acc + (last if sabotage == "no_third" else np.float32(last / np.float32(3))))
            if sabotage == "max_dw":
                last = biggest
            ok = plane_ok and not (acc < min_points or last < min_points)
            valid[k, t] = ok
            if ok:
                score[k, t] = acc if sabotage == "no_min" else min(acc, last)
            decided[k, t] = sure
            exact[k, t] = (lo[1] == hi[1]) and np.array_equal(lo[0][t], hi[0][t])
    return {"counts": counts, "close_plane": plane, "score": score, "valid": valid, "finite": finite, "xlen": xlen,
            "T": Tm, "decided": decided, "exact": exact}


def frames(g, theta=THETA_SEARCH, sabotage=None):
    """The kept frames of a `grade` result in the reference's append order -> dict: `pair`, `roll` (F,),
    `global_to_local` (F, 4, 4) float64 = L2LS[roll] @ T (:218), `search_score` (F,) float32."""
    L = local_to_local_search(theta, sabotage)
    pair, roll = np.nonzero(g["valid"])
    return {"pair": pair, "roll": roll, "global_to_local": L[roll] @ g["T"][pair],
            "search_score": g["score"][pair, roll]}


def nearest(points, global_to_local, sabotage=None, midpoint=None):
    """:79-86: the object point nearest to each frame's centre, the lower index on a tie -> (index (F,), decided (F,):
    the runner-up is further than NEAREST_MARGIN in squared distance)."""
    P = np.asarray(points, np.float64)
    G = np.asarray(global_to_local, np.float64)
    centre = -np.einsum("fji,fj->fi", G[:, :3, :3], G[:, :3, 3])      # the translation of [R^T | -R^T t]
    if sabotage == "nearest_from_midpoint":
        centre = midpoint
    idx = np.zeros(len(G), np.int64)
    sure = np.zeros(len(G), bool)
    for f in range(len(G)):
        d2 = ((P - centre[f]) ** 2).sum(1)
        o = np.argsort(d2, kind="stable")[:2]
        idx[f] = o[0]
        sure[f] = len(o) < 2 or d2[o[1]] - d2[o[0]] > NEAREST_MARGIN
    return idx, sure


def object_data(points, normals, row=None, col=None, eps0=0.0, sabotage=None):
    """All four stages.  row / col: grade these pairs instead of the whole list -> (pairs dict, grade dict, frames dict
    with `frame_point_index`, `point_decided`, `antipodal_score`)."""
    pr = pairs(points, normals, sabotage)
    if row is None:
        row, col = pr["row"], pr["col"]
    g = grade(points, row, col, eps0, sabotage)
    fr = frames(g, sabotage=sabotage)
    P = np.asarray(points, np.float64)
    mid = (P[np.asarray(row)[fr["pair"]]] + P[np.asarray(col)[fr["pair"]]]) / 2
    fr["frame_point_index"], fr["point_decided"] = nearest(points, fr["global_to_local"], sabotage, mid)
    return pr, g, fr
