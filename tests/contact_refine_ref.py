"""The float64 yardstick of the contact-object pipeline's refine and reduce stages: data_gen/utils/
refine_contact_object.py:45-114 and data_gen/utils/smooth_contact_object.py:36-97 restated in numpy, with named
switches that each break one statement (the sabotage tests of tests/test_contact_refine_ref.py).

`refine`: every count in float64 from the inputs as given.  A frame is DECIDED when kept, score and the failure bits
are the same with every region widened and with every region narrowed by `eps`; it is EXACT when every count word is.
`reduce`: integers and one float64 neighbour search; nothing to decide beyond the neighbour order, which `knn_orders_agree`
compares between fp32 and float64."""
import numpy as np

HEIGHT_SEARCH = (-0.01, 0.01, 0)           # refine_contact_object.py:20-23
WIDTH_SEARCH = (0,)
LENGTH_SEARCH = (-0.01, 0.01, 0)
REFINE_MIN_SEARCH_SCORE = 100              # :18
REDUCE_MIN_SEARCH_SCORE = 50               # smooth_contact_object.py:14-16
FRAME_PER_POINT, MAX_NEIGHBOR_FRAME = 5, 4
MIN_REST, RADIUS, MAX_NN = 5, 0.01, 5      # :71-72
HALF_BOTTOM_WIDTH, FINGER_WIDTH = 0.057, 0.023          # data_gen/configs/config.py:50-56
HALF_BOTTOM_SPACE = HALF_BOTTOM_WIDTH - FINGER_WIDTH
HALF_HAND_THICKNESS, BOTTOM_LENGTH, FINGER_LENGTH = 0.012, 0.08, 0.09
FAIL_FINGER, FAIL_FEW, FAIL_BEHIND, FAIL_NONFINITE, FAIL_FILTERED = 1, 2, 4, 8, 16

REFINE_SABOTAGES = ("dy_sign", "behind_le", "count_gt", "last_placement", "drop_heights", "drop_lengths",
                    "prefilter_side")
REDUCE_SABOTAGES = ("rest_first", "own_index", "caps_swapped", "cap_not_reduced", "min_rest_off", "order_by_index")


def local_coordinates(points, g2l):
    """points (N, 3), g2l (F, 4, 4) -> (F, 3, N) float64: rows 0..2 of g2l @ [points; 1]."""
    P = np.asarray(points, np.float64)
    G = np.asarray(g2l, np.float64)
    return G[:, :3, :3] @ P.T[None] + G[:, :3, 3:]


def local_coordinates_f32(points, g2l):
    """The same in fp32, every operation rounded on its own in the order of csrc/frame_sweep.h's local_point."""
    P = np.asarray(points, np.float32)
    G = np.asarray(g2l, np.float32)
    x, y, z = P[None, None, :, 0], P[None, None, :, 1], P[None, None, :, 2]
    g = G[:, :3, :, None]
    return ((g[:, :, 0] * x + g[:, :, 1] * y) + g[:, :, 2] * z) + g[:, :, 3]


def _counts(L, e, heights, widths, lengths, sabotage):
    x, y, z = L[:, 0], L[:, 1], L[:, 2]
    F = L.shape[0]
    out = np.zeros((F, len(heights) * len(widths) * len(lengths), 3), np.int64)
    p = 0
    for dz in heights:                                                           # :74, dz outer
        zb = (z < HALF_HAND_THICKNESS + dz + e) & (z > -HALF_HAND_THICKNESS + dz - e)
        for dy in widths:
            yb = (y < HALF_BOTTOM_SPACE + dy + e) & (y > -HALF_BOTTOM_SPACE + dy - e)     # :78-79
            ay = np.abs(y - dy) if sabotage == "dy_sign" else np.abs(y + dy)              # :80
            yc = (ay > HALF_BOTTOM_SPACE - e) & (ay < HALF_BOTTOM_WIDTH + e)              # :81
            for dx in lengths:
                xb = (x > -BOTTOM_LENGTH + dx - e) & (x < FINGER_LENGTH + dx + e)         # :84-85
                close = xb & zb & yb                                                      # :89
                behind = (x <= e) if sabotage == "behind_le" else (x < e)                 # :93
                out[:, p, 0] = (zb & xb & yc).sum(1)                                      # :86-87
                out[:, p, 1] = close.sum(1)
                out[:, p, 2] = (close & behind).sum(1)
                p += 1
    return out


def _verdict(counts, min_search, threshold, sabotage):
    fing, close, behind = counts[..., 0], counts[..., 1], counts[..., 2]
    few = (close <= min_search) if sabotage == "count_gt" else (close < min_search)       # :91
    fail = (np.where((fing > threshold).any(1), FAIL_FINGER, 0) | np.where(few.any(1), FAIL_FEW, 0) |
            np.where((behind > 0).any(1), FAIL_BEHIND, 0))
    score = close[:, -1] if sabotage == "last_placement" else close.min(1)                # :95
    return fail, np.where(fail == 0, score, 0)


def refine(points, g2l, search_score, min_search_score=REFINE_MIN_SEARCH_SCORE, collision_threshold=0,
           heights=HEIGHT_SEARCH, widths=WIDTH_SEARCH, lengths=LENGTH_SEARCH, eps=0.0, sabotage=None, block=256):
    """-> dict: `live` (F,) bool the pre-filter, `counts` (F, P, 3) int64 {finger, close, behind} (zero on rows that
    are not live or not finite), `fail` (F,) the bits, `kept` (F,) bool, `score` (F,) int64 (0 where not kept),
    `kept_index` the kept rows ascending, `decided`, `exact` (F,) bool."""
    if sabotage == "drop_heights":
        heights = (0,)
    if sabotage == "drop_lengths":
        lengths = (0,)
    G = np.asarray(g2l, np.float64)
    s = np.asarray(search_score, np.float64)
    F = len(G)
    live = (s < min_search_score) if sabotage == "prefilter_side" else (s > min_search_score)        # :46
    finite = np.isfinite(G.reshape(F, 16)).all(1)
    scan = np.nonzero(live & finite)[0]
    P = len(heights) * len(widths) * len(lengths)
    counts = np.zeros((F, P, 3), np.int64)
    fail = np.where(live, np.where(finite, 0, FAIL_NONFINITE), FAIL_FILTERED).astype(np.int64)
    score = np.zeros(F, np.int64)
    decided = np.ones(F, bool)
    exact = np.ones(F, bool)
    with np.errstate(invalid="ignore"):
        for b0 in range(0, len(scan), block):
            rows = scan[b0:b0 + block]
            L = local_coordinates(points, G[rows])
            c = _counts(L, 0.0, heights, widths, lengths, sabotage)
            counts[rows] = c
            fail[rows], score[rows] = _verdict(c, min_search_score, collision_threshold, sabotage)
            if eps > 0.0:
                for e in (eps, -eps):
                    ce = _counts(L, e, heights, widths, lengths, sabotage)
                    fe, se = _verdict(ce, min_search_score, collision_threshold, sabotage)
                    decided[rows] &= (fe == fail[rows]) & (se == score[rows])
                    exact[rows] &= (ce == c).all((1, 2))
    kept = fail == 0
    return {"live": live, "counts": counts, "fail": fail, "kept": kept, "score": score,
            "kept_index": np.nonzero(kept)[0], "decided": decided, "exact": exact}


def knn(points, i, radius=RADIUS, max_nn=MAX_NN, dtype=np.float64):
    """open3d's search_hybrid_vector_3d as the library pins it: the max_nn smallest (squared distance, index) of the
    points with d^2 < r^2.  dtype float32: the kernel's arithmetic ((dx dx + dy dy) + dz dz, r^2 the fp32 product)."""
    P = np.asarray(points, dtype)
    d = P - P[i]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r2 = dtype(radius) * dtype(radius)
    with np.errstate(invalid="ignore"):
        idx = np.nonzero(d2 < r2)[0]
    return idx[np.lexsort((idx, d2[idx]))][:max_nn]


def knn_orders_agree(points, queries, radius=RADIUS, max_nn=MAX_NN):
    return all(np.array_equal(knn(points, i, radius, max_nn), knn(points, i, radius, max_nn, np.float32))
               for i in queries)


def reduce(points, frame_point_index, search_score, min_search_score=REDUCE_MIN_SEARCH_SCORE,
           frame_per_point=FRAME_PER_POINT, max_neighbor_frame=MAX_NEIGHBOR_FRAME, min_rest=MIN_REST, radius=RADIUS,
           max_nn=MAX_NN, sabotage=None, neighbours=None):
    """-> dict: `source_frame`, `point_index` (K,) int64 in the script's append order (source_frame indexes the rows
    as given, before the filter), `stats` the branch counts, `queries` the points whose neighbours were searched.
    neighbours: a function i -> indices replacing the float64 search (the GPU tests pass the library's own)."""
    P = np.asarray(points, np.float64)
    N = len(P)
    fpi = np.asarray(frame_point_index).astype(np.int64)
    valid = np.nonzero(np.asarray(search_score) > min_search_score)[0]                  # :37
    fp = fpi[valid]
    order = np.argsort(fp, kind="stable")
    lo, hi = np.searchsorted(fp[order], np.arange(N)), np.searchsorted(fp[order], np.arange(N), side="right")
    if sabotage == "min_rest_off":
        min_rest = min_rest + 1
    pfn = np.zeros(N, np.int64)
    src, pts, queries = [], [], []
    st = dict(over=0, long_rest=0, spread=0, denied_lower=0, denied_higher=0, capped_elif=0, holding=0)
    for i in range(N):
        pf = valid[order[lo[i]:hi[i]]]                                                   # :62, ascending frame index
        if len(pf) == 0:
            continue
        st["holding"] += int(pfn[i] > 0)
        room = frame_per_point if sabotage == "cap_not_reduced" else frame_per_point - pfn[i]
        if len(pf) > frame_per_point:                                                    # :63
            st["over"] += 1
            new = pf[0:room]                                                             # :64
            src.extend(new)
            pts.extend([i] * len(new))
            pfn[i] += len(new)
            rest = pf[frame_per_point:]                                                  # :70
            if len(rest) > min_rest:                                                     # :71
                st["long_rest"] += 1
                queries.append(i)
                idx = knn(P, i, radius, max_nn) if neighbours is None else neighbours(i)
                if sabotage == "order_by_index":
                    idx = np.sort(idx)
                for r, n in enumerate(idx):                                              # :73
                    n = int(n)
                    lower_cap, higher_cap = frame_per_point, max_neighbor_frame
                    if sabotage == "caps_swapped":
                        lower_cap, higher_cap = higher_cap, lower_cap
                    if (n < i and pfn[n] < lower_cap) or (n > i and pfn[n] < higher_cap):            # :75-76
                        pfn[n] += 1
                        src.append(rest[0] if sabotage == "rest_first" else rest[r])     # :78
                        pts.append(i if sabotage == "own_index" else n)                  # :81
                        st["spread"] += 1
                    elif n < i:
                        st["denied_lower"] += 1
                    elif n > i:
                        st["denied_higher"] += 1
        else:
            added = min(room, len(pf))                                                   # :84
            st["capped_elif"] += int(added < len(pf))
            src.extend(pf[:added])
            pts.extend([i] * added)
            pfn[i] += added
    return {"source_frame": np.array(src, np.int64), "point_index": np.array(pts, np.int64), "stats": st,
            "queries": np.array(queries, np.int64)}
