"""The operators' double dispatch (csrc/ops_f64.hip) at its kernel edges.  Plain data and numpy: the case tables with
every loop constant T of those kernels as T - 1, T, T + 1, the seeded inputs the cases run on, float64 numpy models of
every operator written from the reference's statements (sampling_kernel.cu:49-119, ball_query_kernel.cu:33-76,
interpolate_kernel.cu:32-81 / 138-181 / 243-286, grouping_kernel.cu:32-96) -- a second witness beside the C oracle --
and, through `sab=`, wrong-kernel variants of those models.  tests/test_f64_edges.py keeps the tables honest against
the source and shows that the inputs see every variant; tests/test_f64_edges_gpu.py runs the cases on the GPU.

A case is a dict; "op" names the operator, the sizes follow, "kind" names the input construction.  Every input has
B = 3 scenes: the B = 1 runs are its scenes one at a time."""
import numpy as np

from tests.dispatch_edges import lattice_levels, seed_of

# ------------------------------------------------------------------------------------------------------ constants
# (tests/test_f64_edges.py reads each of them out of csrc/ops_f64.hip and fails when one moves)
F64_FPS_THREADS = 1024          # fps_f64_kernel: threads of the one workgroup per scene
FPS_LG_MIN, FPS_LG_MAX = 4, 9   # ref_block_lg_f64: the bit count of the tie key's reversed part
BQ_WAVES = 4                    # ball_query_f64_kernel: centroids (waves) per workgroup
BQ_STEP = 64                    # ... points per step of a wave
EW_THREADS = 256                # three_nn / group / interpolate / backward: one element per thread, 256 per block
NN_SENTINEL = 1e40              # interpolate_kernel.cu:53: finite in double
B = 3

EPS40 = 2.0 ** -40
RADIUS = 0.25                   # r and r r exact


# ------------------------------------------------------------------------------------------------------ tables
FPS_N = [1, 2, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
FPS_KINDS = ("uniform64", "lattice", "double_only")
FPS_FMAD_N = [16, 512, 1024, 2049]           # one N per regime: lg clamped up, lg = ceil log2 N, one point per thread, two or more
BQ_N = [1, 63, 64, 65, 127, 128, 129, 1000]
BQ_M = [1, 2, 3, 4, 5, 301]
BQ_K = [1, 2, 63, 64, 65, 200]
BQ_KINDS = ("empty", "last", "lane63", "straddle", "late", "short_pad", "exact_r", "natural")
NN_N1 = [1, 255, 256, 257, 1001]
NN_N2 = [3, 4, 5, 64, 1000]
NN_KINDS = ("uniform64", "lattice", "double_only", "coincident", "sentinel", "nonfinite")
EW_S = [1, 255, 256, 257, 1000]              # M K of group / gather and their backward, N1 of interpolate and its backward
EW_C = [1, 3]
EW_N = [1, 7, 300]                           # the gathered / scattered extent N, N2
EW_OPS = ("group", "gather", "interp", "group_bwd", "interp_bwd")


def fps_ms(N):
    """M = N, M = 1 and one in between."""
    return sorted({N, 1, max(1, min(N - 1, max(3, N // 2)))}, reverse=True)


def fps_cases():
    out = []
    for N in FPS_N:
        for M in fps_ms(N):
            for kind in FPS_KINDS:
                out.append(dict(op="fps", N=N, M=M, kind=kind, fmad=0))
    for N in FPS_FMAD_N:
        for kind in ("uniform64", "lattice"):
            out.append(dict(op="fps", N=N, M=max(1, N // 2), kind=kind, fmad=1))
    out.append(dict(op="fps", N=257, M=257, kind="coincident", fmad=0))
    out.append(dict(op="fps", N=1025, M=9, kind="coincident", fmad=1))
    out.append(dict(op="fps", N=130, M=12, kind="nonfinite", fmad=0))
    return out


def bq_cases():
    rows = [(1, 1, 1, "last"), (1, 2, 2, "empty"), (63, 3, 2, "last"), (63, 4, 63, "exact_r"), (64, 5, 2, "lane63"),
            (128, 4, 64, "lane63"), (65, 3, 1, "straddle"), (129, 2, 63, "straddle"), (127, 301, 65, "empty"),
            (128, 5, 200, "short_pad"), (129, 2, 64, "late"), (1000, 301, 200, "late"), (1000, 5, 65, "lane63"),
            (1000, 3, 64, "exact_r"), (65, 1, 2, "last"), (127, 2, 1, "natural"), (1000, 4, 63, "natural"),
            (1000, 5, 2, "straddle")]
    out = [dict(op="bq", N=N, M=M, K=K, kind=kind, fmad=0) for N, M, K, kind in rows]
    out.append(dict(op="bq", N=1000, M=5, K=64, kind="exact_r", fmad=1))
    out.append(dict(op="bq", N=129, M=3, K=63, kind="nonfinite", fmad=0))
    return out


def nn_cases():
    rows = [(1, 3, "uniform64"), (255, 4, "lattice"), (256, 5, "uniform64"), (257, 64, "double_only"),
            (1001, 1000, "uniform64"), (257, 1000, "lattice"), (256, 64, "double_only"), (1, 1000, "lattice"),
            (255, 3, "coincident"), (257, 64, "sentinel"), (255, 3, "sentinel"), (257, 5, "nonfinite")]
    out = [dict(op="nn", N1=N1, N2=N2, kind=kind, fmad=0) for N1, N2, kind in rows]
    out += [dict(op="nn", N1=257, N2=64, kind=kind, fmad=1) for kind in ("uniform64", "sentinel", "double_only")]
    return out


def ew_cases():
    """The one-element-per-thread kernels: S = M K or N1 on the block ladder at (C, N) = (3, 300) and (1, 7), the hot
    target N = 1 at S = 257, and a NaN / inf feature row."""
    out = []
    for op in EW_OPS:
        fmads = (0, 1) if op == "interp" else (0,)
        for fmad in fmads:
            for S in EW_S:
                out.append(dict(op=op, S=S, C=3, N=300, kind="plain", fmad=fmad))
                out.append(dict(op=op, S=S, C=1, N=7, kind="plain", fmad=fmad))
            out.append(dict(op=op, S=257, C=3, N=1, kind="hot", fmad=fmad))
            if op.endswith("_bwd"):
                out.append(dict(op=op, S=257, C=3, N=300, kind="hot", fmad=fmad))
            else:
                out.append(dict(op=op, S=257, C=3, N=7, kind="nonfinite", fmad=fmad))
        if op == "interp":
            out.append(dict(op=op, S=257, C=3, N=7, kind="signed_zero", fmad=0))
            out.append(dict(op=op, S=257, C=3, N=7, kind="signed_zero", fmad=1))
    return out


def all_cases():
    return fps_cases() + bq_cases() + nn_cases() + ew_cases()


def case_id(c):
    parts = [c["op"]]
    for k in ("N", "M", "K", "N1", "N2", "S", "C"):
        if k in c:
            parts.append("%s=%d" % (k, c[k]))
    parts.append(c["kind"])
    if c.get("fmad"):
        parts.append("fmad")
    return "-".join(parts)


def mk_of(c):
    """(M, K) of a grouping case: K = 1 through gather_points."""
    S = c["S"]
    if c["op"] == "gather":
        return S, 1
    for K in (4, 3, 2):
        if S % K == 0:
            return S // K, K
    return S, 1


# ------------------------------------------------------------------------------------------------------ arithmetic
def fma64(a, b, c):
    """fl64(a b + c) with ONE rounding for float64 arrays (Boldo and Melquiond, "Emulation of a FMA and correctly
    rounded sums: proved algorithms using rounding to odd"): a b = uh + ul exactly (Dekker), c + uh = th + tl exactly
    (Knuth), v = tl + ul rounded to odd, result th + v.  Non-finite operands take the plain expression (no rounding is
    involved in their result).  Valid while neither the split (|x| < 2^996) nor the low product underflows: the inputs
    of this module stay within 1e-30 .. 1e43."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(all="ignore"):
        uh = a * b
        plain = uh + c
        sa = a * 134217729.0
        ah = sa - (sa - a)
        al = a - ah
        sb = b * 134217729.0
        bh = sb - (sb - b)
        bl = b - bh
        ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl
        th = c + uh
        t = th - c
        tl = (c - (th - t)) + (uh - t)
        v = tl + ul
        t2 = v - tl
        err = (tl - (v - t2)) + (ul - t2)
        even = (v.view(np.int64) & 1) == 0
        v = np.where((err != 0) & even, np.nextafter(v, np.where(err > 0, np.inf, -np.inf)), v)
        z = th + v
    ok = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(plain)
    return np.where(ok, z, plain)


def dist2_64(x1, y1, z1, x2, y2, z2, fmad=0, sab=None):
    """(x2 - x1)^2 + (y2 - y1)^2 + (z2 - z1)^2 left to right, every operation rounded to double; fmad: the contraction
    fma(dz, dz, fma(dy, dy, dx dx)) of include/s4g_ops.h's distance contract."""
    with np.errstate(all="ignore"):
        dx, dy, dz = x2 - x1, y2 - y1, z2 - z1
        if sab == "f32_diff":
            dx, dy, dz = (v.astype(np.float32).astype(np.float64) for v in (dx, dy, dz))
        d = fma64(dz, dz, fma64(dy, dy, dx * dx)) if fmad else (dx * dx + dy * dy) + dz * dz
        if sab == "f32_dist":
            d = d.astype(np.float32).astype(np.float64)
    return d


def _bitrev(v, bits):
    r = np.zeros_like(v)
    for _ in range(bits):
        r = (r << 1) | (v & 1)
        v = v >> 1
    return r


def ceil_log2(n):
    cnt, x = 0, n - 1
    while x > 0:
        x >>= 1
        cnt += 1
    return cnt


def fps_lg(N, clamp=True):
    """log2 of the reference's block size: get_block() (sampling_kernel.cu:34-42) and the switch's 16-thread floor."""
    lg = ceil_log2(N)
    return min(max(lg, FPS_LG_MIN), FPS_LG_MAX) if clamp else lg


# ------------------------------------------------------------------------------------------------------ models
FPS_SABOTAGES = {
    "f32_coords": "coordinates rounded to fp32",
    "tie_lowest_index": "a tie goes to the lowest index instead of the lowest composite key",
    "no_clamp": "lg_bs without the 4 / 9 clamp",
    "skip_1024": "points j >= 1024 skipped",
    "min_not_stored": "the running minimum not stored",
    "no_d_guard": "the d > 0 guard of the tie rule dropped",
}
BQ_SABOTAGES = {
    "le": "<= for <",
    "pad_zero": "padding with 0 instead of the first hit",
    "tail_read": "N rounded up to a multiple of 64: the tail lanes read on",
    "f32_dist": "distance rounded to fp32",
    "cnt_unclamped": "the count not clamped to K",
}
NN_SABOTAGES = {
    "le": "<= for <",
    "f32_dist": "distance rounded to fp32",
    "inf_sentinel": "sentinel +inf instead of 1e40",
    "minus1": "the -1 initialiser written through",
}
EW_SABOTAGES = {
    "batch_offset": "the batch offset of the index dropped",
    "chan_extent": "the channel offset of the source taken from the wrong extent",
    "last_block": "the last partial block of 256 dropped",
    "weights_rotated": "the three weights rotated",
    "assoc_swapped": "the fmad / strict association swapped",
}
NOT_WRITTEN = np.nan


def fps_np(pts, M, fmad=0, sab=None, ties=None):
    """FarthestPointSampleKernel on (B, 3, N) float64 -> (B, M) int64.  Per step: temp[j] = dist where temp[j] > dist or
    temp[j] < 0, else dist = temp[j] (:85-90); the winner is the greatest dist > 0, and among equal ones the thread /
    halving-tree order, in closed form the lowest (bitreverse_lg(j mod 2^lg), j); nothing > 0: the index repeats.
    `ties`, a dict, collects what the steps' ties looked like."""
    if sab == "f32_coords":
        pts = pts.astype(np.float32).astype(np.float64)
    nb, _, N = pts.shape
    lg = fps_lg(N, clamp=sab != "no_clamp")
    j = np.arange(N, dtype=np.int64)
    key = j if sab == "tie_lowest_index" else (_bitrev(j & ((1 << lg) - 1), lg) << 23) | j
    out = np.zeros((nb, M), np.int64)
    for b in range(nb):
        x, y, z = pts[b]
        temp = np.full(N, -1.0)
        cur = 0
        for i in range(1, M):
            dist = dist2_64(x[cur], y[cur], z[cur], x, y, z, fmad)
            with np.errstate(invalid="ignore"):
                upd = (temp > dist) | (temp < 0)
                d = np.where(upd, dist, temp)
                if sab != "min_not_stored":
                    temp = d
                cand = d >= 0 if sab == "no_d_guard" else d > 0
            if sab == "skip_1024":
                cand = cand & (j < F64_FPS_THREADS)
            if cand.any():
                top = d[cand].max()
                tied = j[cand & (d == top)]
                cur = int(tied[np.argmin(key[tied])])
                if ties is not None and len(tied) > 1 and top > 0:
                    t = tied % F64_FPS_THREADS
                    ties["waves"] = ties.get("waves", False) or len(set(t // 64)) > 1
                    ties["strides"] = ties.get("strides", False) or bool(np.isin(tied + F64_FPS_THREADS, tied).any())
                    ties["count"] = ties.get("count", 0) + 1
            out[b, i] = cur
    return out


def ball_query_np(pts, ctr, radius, K, fmad=0, sab=None):
    """BallQueryKernel on (B, 3, N) / (B, 3, M) float64 -> (index (B, M, K), count (B, M)) int64: points in index order
    while cnt < K, strict dist < r r (r a C float cast to double), the first hit fills all K slots, zeros without one."""
    nb, _, N = pts.shape
    M = ctr.shape[2]
    r = np.float64(np.float32(radius))
    r2 = r * r
    idx = np.zeros((nb, M, K), np.int64)
    cnt = np.zeros((nb, M), np.int64)
    flat = np.concatenate([pts.reshape(-1), np.zeros(3 * BQ_STEP)])
    for b in range(nb):
        n = N
        x, y, z = pts[b]
        if sab == "tail_read":
            n = -(-N // BQ_STEP) * BQ_STEP
            o = b * 3 * N
            x, y, z = flat[o:o + n], flat[o + N:o + N + n], flat[o + 2 * N:o + 2 * N + n]
        for m in range(M):
            d = dist2_64(ctr[b, 0, m], ctr[b, 1, m], ctr[b, 2, m], x, y, z, fmad, sab)
            with np.errstate(invalid="ignore"):
                hits = np.nonzero(d <= r2 if sab == "le" else d < r2)[0]
            take = hits[:K]
            if len(take):
                idx[b, m, :] = 0 if sab == "pad_zero" else take[0]
                idx[b, m, :len(take)] = take
            cnt[b, m] = len(take)
            if sab == "cnt_unclamped" and len(hits) >= K:
                cnt[b, m] = (hits < (take[K - 1] // BQ_STEP + 1) * BQ_STEP).sum()     # to the end of the step that reached K
    return idx, cnt


def three_nn_np(q, k, fmad=0, sab=None):
    """PointSearchKernel on (B, 3, N1) / (B, 3, N2) float64 -> (index (B, N1, 3) int64, squared distance (B, N1, 3)):
    min_dist = {1e40, 0, 0}, min_ind = {-1, 0, 0}, keys in index order, insertion at the first slot with d < min_dist
    (:63-73).  The library's documented index rule: a slot that still holds the initialiser -1 reports index 0."""
    nb, _, N1 = q.shape
    N2 = k.shape[2]
    dist = np.zeros((nb, N1, 3))
    dist[:, :, 0] = np.inf if sab == "inf_sentinel" else NN_SENTINEL
    ind = np.zeros((nb, N1, 3), np.int64)
    ind[:, :, 0] = -1
    lt = (lambda a, b: a <= b) if sab == "le" else (lambda a, b: a < b)
    for j in range(N2):
        # (x1 - x2)^2 is (x2 - x1)^2 bit for bit
        d = dist2_64(k[:, 0, j, None], k[:, 1, j, None], k[:, 2, j, None], q[:, 0], q[:, 1], q[:, 2], fmad, sab)
        with np.errstate(invalid="ignore"):
            c0 = lt(d, dist[:, :, 0])
            c1 = ~c0 & lt(d, dist[:, :, 1])
            c2 = ~c0 & ~c1 & lt(d, dist[:, :, 2])
        for a, src in ((dist, d), (ind, j)):
            a2 = np.where(c0 | c1, a[:, :, 1], np.where(c2, src, a[:, :, 2]))
            a1 = np.where(c0, a[:, :, 0], np.where(c1, src, a[:, :, 1]))
            a0 = np.where(c0, src, a[:, :, 0])
            a[:, :, 0], a[:, :, 1], a[:, :, 2] = a0, a1, a2
    if sab != "minus1":
        ind = np.where(ind < 0, 0, ind)
    return ind, dist


def _flat_index(idx, sab):
    nb = idx.shape[0]
    ix = idx.reshape(nb, -1)
    return np.broadcast_to(ix[:1], ix.shape) if sab == "batch_offset" else ix


def _source(feat, S, sab):
    """(B, C, N) rows as the kernel addresses them; "chan_extent": row (b, c) starts at (b C + c) S instead of (b C + c) N."""
    nb, C, N = feat.shape
    if sab != "chan_extent":
        return feat
    flat = feat.reshape(-1)
    start = (np.arange(nb * C) * S)[:, None] + np.arange(N)[None, :]
    return flat[start % flat.size].reshape(nb, C, N)


def _drop_last_block(out, sab):
    S = out.shape[2]
    if sab == "last_block" and S % EW_THREADS:
        out[:, :, EW_THREADS * (S // EW_THREADS):] = NOT_WRITTEN
    return out


def group_points_np(feat, idx, sab=None):
    """out[b, c, m, k] = in[b, c, idx[b, m, k]] (grouping_kernel.cu:32-54); idx (B, M, K), or (B, M) for gather_points."""
    nb, C, N = feat.shape
    ix = _flat_index(idx, sab)
    src = _source(feat, ix.shape[1], sab)
    out = np.take_along_axis(src, np.broadcast_to(ix[:, None, :], (nb, C, ix.shape[1])), axis=2).copy()
    return _drop_last_block(out, sab).reshape((nb, C) + idx.shape[1:])


def three_interpolate_np(feat, idx, w, fmad=0, sab=None):
    """acc = 0; acc += in[idx_k] w_k, k = 0, 1, 2 (interpolate_kernel.cu:160-174): every product and sum rounded
    (strict) or acc = fma(in, w, acc) (fmad).  The sum starts from +0.0."""
    nb, C, N2 = feat.shape
    N1 = idx.shape[1]
    ix = np.broadcast_to(idx[:1], idx.shape) if sab == "batch_offset" else idx
    ww = np.roll(w, 1, axis=2) if sab == "weights_rotated" else w
    src = _source(feat, N1, sab)
    if sab == "assoc_swapped":
        fmad = not fmad
    acc = np.zeros((nb, C, N1))
    with np.errstate(all="ignore"):
        for k in range(3):
            g = np.take_along_axis(src, np.broadcast_to(ix[:, None, :, k], (nb, C, N1)), axis=2)
            wk = np.broadcast_to(ww[:, None, :, k], (nb, C, N1))
            acc = fma64(g, wk, acc) if fmad else acc + g * wk
    return _drop_last_block(acc, sab)


def _scatter(contrib, ix, N, sab):
    """gin[b, c, ix[b, t]] += contrib[b, c, t] in ascending t (the oracle's order; the kernel's atomics have none)."""
    nb, C, T = contrib.shape
    gin = np.zeros((nb, C, N))
    keep = T if not (sab == "last_block" and T % EW_THREADS) else EW_THREADS * (T // EW_THREADS)
    for b in range(nb):
        for c in range(C):
            np.add.at(gin[b, c], ix[b, :keep], contrib[b, c, :keep])
    return gin


def group_points_backward_np(gout, idx, N, sab=None):
    """gin[b, c, idx[b, m, k]] += gout[b, c, m, k] (grouping_kernel.cu:57-96)."""
    nb, C = gout.shape[:2]
    ix = _flat_index(idx, sab)
    g = gout.reshape(nb, C, -1)
    return _scatter(_source(g, N, sab) if sab == "chan_extent" else g, ix, N, sab)


def three_interpolate_backward_np(gout, idx, w, N2, sab=None):
    """gin[b, c, idx[b, n, k]] += gout[b, c, n] w[b, n, k] (interpolate_kernel.cu:272-286), the product rounded."""
    nb, C, N1 = gout.shape
    ix = np.broadcast_to(idx[:1], idx.shape) if sab == "batch_offset" else idx
    ww = np.roll(w, 1, axis=2) if sab == "weights_rotated" else w
    g = _source(gout, N2, sab) if sab == "chan_extent" else gout
    if sab == "last_block" and N1 % EW_THREADS:
        keep = EW_THREADS * (N1 // EW_THREADS)
        g, ix, ww, N1 = g[:, :, :keep], ix[:, :keep], ww[:, :keep], keep
    contrib = (g[:, :, :, None] * ww[:, None, :, :]).reshape(nb, C, 3 * N1)
    return _scatter(contrib, ix.reshape(nb, -1), N2, None)


def interp_weights_np(d2, eps=1e-10):
    """modules.py:118-120: inv = 1 / clamp(d2, min=eps); w = inv / sum_k inv."""
    inv = 1.0 / np.maximum(d2, eps)
    return inv / ((inv[:, :, 0] + inv[:, :, 1]) + inv[:, :, 2])[:, :, None]


# ------------------------------------------------------------------------------------------------------ inputs
def _rng(c, *extra):
    return np.random.default_rng(seed_of(*(int(v) for k, v in sorted(c.items()) if isinstance(v, (int, np.integer))),
                                         len(c["op"]), len(c["kind"]), *extra))


def uniform64(rng, shape):
    """Doubles that no float holds: a random fp32 value plus a perturbation near 2^-40 of its magnitude."""
    base = rng.random(shape, dtype=np.float32).astype(np.float64) + 2.0 ** -12
    out = base * (1.0 + EPS40 * (1.0 + rng.random(shape)))
    assert (out.astype(np.float32).astype(np.float64) != out).all()
    return out


def lattice64(rng, nb, N):
    """dispatch_edges.lattice_cloud in double: a 2^-5 lattice with fewer positions than points."""
    return rng.integers(0, lattice_levels(N), size=(nb, 3, N)).astype(np.float64) * 0.03125


FPS_CORNERS = ((4.0, 4.0, 4.0), (-4.0, 4.0, 4.0), (4.0, -4.0, 4.0))


def fps_pairs(N):
    """[(a, b)]: index pairs placed on one far corner each -- equal maxima by construction.  (5, 69) sit in different
    waves, (7, 7 + 1024) in different strides of one thread, (1, 2) in one wave."""
    out = []
    for a, b in ((5, 69), (7, 7 + F64_FPS_THREADS), (1, 2)):
        if b < N and N >= 4:
            out.append((a, b))
    return out


def fps_tie_key(N, j):
    lg = fps_lg(N)
    return (int(_bitrev(np.int64(j) & ((1 << lg) - 1), lg)) << 23) | j


def fps_inputs(c):
    """(B, 3, N) float64.  "lattice": the coarse lattice plus the corner pairs of fps_pairs; "double_only": the same
    with the point of each pair that the tie key does NOT prefer moved outward by 2^-40 of its coordinates: strictly
    farther in double, so it is picked; tied again once rounded to fp32, where the key picks the other."""
    N, kind = c["N"], c["kind"]
    rng = _rng(c)
    if kind in ("uniform64", "nonfinite"):
        pts = uniform64(rng, (B, 3, N))
        if kind == "nonfinite":
            pts[:, 0, 3] = np.nan
            pts[:, 1, 5] = np.inf
        return pts
    if kind == "coincident":
        return np.broadcast_to(uniform64(rng, (B, 3, 1)), (B, 3, N)).copy()
    pts = lattice64(rng, B, N)
    for (a, b), corner in zip(fps_pairs(N), FPS_CORNERS):
        moved = b if fps_tie_key(N, a) < fps_tie_key(N, b) else a
        for i in (a, b):
            pts[:, :, i] = np.array(corner) * ((1.0 + 2.0 ** -40) if kind == "double_only" and i == moved else 1.0)
    return pts


BQ_CENTRE = np.array([0.5, 0.5, 3.5])       # the constructed ball's centroid: 2 away from every background point


def bq_hits(c):
    """The indices the constructed ball holds, by kind -> (inside, on_the_sphere)."""
    N, K, kind = c["N"], c["K"], c["kind"]
    step = BQ_STEP
    if kind == "last":
        return [N - 1], []
    if kind == "lane63":                      # exactly K hits, the K-th on lane 63 of the last full step
        last = step * (N // step) - 1
        assert last - K + 1 >= 0
        return list(range(last - K + 1, last + 1)), []
    if kind == "straddle":                    # K - 1 hits, then a step that holds three more
        s = -(-(K - 1) // step)
        hits = list(range(K - 1)) + [step * s + 1, step * s + 2, step * s + 5]
        assert hits[-1] < N
        return hits, []
    if kind == "late":                        # K hits, then two more in a later step
        assert step * (-(-K // step)) <= N - 2
        return list(range(K)) + [N - 2, N - 1], []
    if kind == "short_pad":
        hits = [N // 2, N - 1]
        assert K - len(hits) > step                       # the padding loop strides
        return hits, []
    if kind == "exact_r":                     # alternately at r (1 - 2^-40) and at r exactly
        js = list(range(1, min(N, 40), 2))
        return js[0::2], js[1::2]
    return [], []


def bq_inputs(c):
    """(points (B, 3, N), centroids (B, 3, M), radius).  Background points are uniform64 in the unit cube; all centroids
    but the last are background points; the last is BQ_CENTRE (far from the background), and the points bq_hits names
    are placed around it -- inside by a random offset of length <= 0.2, at r (1 - 2^-40) or at r exactly along an axis.
    Of an "empty" case every centroid is moved 50 away."""
    N, M, kind = c["N"], c["M"], c["kind"]
    rng = _rng(c)
    pts = uniform64(rng, (B, 3, N))
    inside, sphere = bq_hits(c)
    for b in range(B):
        for n, j in enumerate(inside):
            if kind == "exact_r":
                off = np.zeros(3)
                off[n % 3] = RADIUS * (1.0 - EPS40) * (1 if n % 2 else -1)
            else:
                v = rng.standard_normal(3)
                off = v / np.linalg.norm(v) * 0.2 * rng.random()
            pts[b, :, j] = BQ_CENTRE + off
        for n, j in enumerate(sphere):
            off = np.zeros(3)
            off[n % 3] = RADIUS * (1 if n % 2 else -1)
            pts[b, :, j] = BQ_CENTRE + off
    free = np.setdiff1d(np.arange(N), inside + sphere)
    ctr = np.empty((B, 3, M))
    for b in range(B):
        pick = rng.choice(free if len(free) else np.arange(N), M)
        ctr[b] = pts[b][:, pick]
        if not len(free):
            ctr[b, 2] += 50.0
        ctr[b, :, M - 1] = BQ_CENTRE
    if kind == "empty":
        ctr[:, 0] += 50.0
    if kind == "nonfinite":
        pts[:, 0, 2] = np.nan
        pts[:, 2, 4] = np.inf
        ctr[:, 1, 0] = np.nan
    return pts, ctr, RADIUS


def nn_inputs(c):
    """(queries (B, 3, N1), keys (B, 3, N2)) float64."""
    N1, N2, kind = c["N1"], c["N2"], c["kind"]
    rng = _rng(c)
    if kind == "coincident":
        p = uniform64(rng, (B, 3, 1))
        return np.broadcast_to(p, (B, 3, N1)).copy(), np.broadcast_to(p, (B, 3, N2)).copy()
    if kind in ("lattice", "double_only"):
        levels = lattice_levels(max(N2, 36))
        q = rng.integers(0, levels, size=(B, 3, N1)).astype(np.float64) * 0.03125
        k = rng.integers(0, levels, size=(B, 3, N2)).astype(np.float64) * 0.03125
        if kind == "double_only":
            # every odd key a copy of the key before it, 2^-40 to the right: nearer by less than fp32 resolves to every
            # query right of it, and the LATER of the two
            k[:, :, 1::2] = k[:, :, 0:2 * (N2 // 2):2]
            k[:, 0, 1::2] += EPS40
        return q, k
    q, k = uniform64(rng, (B, 3, N1)), uniform64(rng, (B, 3, N2))
    if kind == "sentinel":
        # keys 1e21 away (squared distance 1e42 >= 1e40): two of them in scene 0, one in scene 1, none in scene 2;
        # query 0 sits beside them, the last query 1e21 away from every key of its scene
        k[0, :, 1] = (1e21, 0.0, 0.0)
        k[0, :, N2 - 1] = (1e21, 3.0, 0.0)
        k[1, :, 2] = (1e21, 0.0, 0.0)
        q[:, :, 0] = (1e21, 1.0, 0.0)
        q[:, :, N1 - 1] = (-1e21, 1e21, 0.0)
    if kind == "nonfinite":
        k[:, 0, 1] = np.nan
        k[:, 1, 3] = np.inf
        q[:, 2, 2] = np.nan
        q[:, 0, 4] = -np.inf
    return q, k


EXACT_WEIGHTS = np.array([0.25, 0.5, 1.0, 2.0])
EXACT_MAX = 64


def make_index(rng, nb, T, N, hot=False):
    """(nb, T) int64 in [0, N): every scene holds 0 and N - 1; "hot": every position names one target."""
    if hot:
        return np.repeat(((np.arange(nb) * 5 + N - 1) % N)[:, None], T, axis=1).astype(np.int64)
    ix = rng.integers(0, N, size=(nb, T), dtype=np.int64)
    for b in range(nb):
        ends = (0, N - 1) if b % 2 == 0 else (N - 1, 0)
        ix[b, 0] = ends[0]
        if T >= 2:
            ix[b, 1] = ends[1]
        if T >= 3:
            ix[b, T - 1] = (ix[b, T - 2] + 1 + b) % N
    return ix


def _values(rng, shape, family):
    if family == "exact":
        return rng.integers(-EXACT_MAX, EXACT_MAX + 1, size=shape).astype(np.float64)
    if family == "natural":                   # magnitudes across e^+-6, no float holds them
        return rng.standard_normal(shape) * np.exp(rng.uniform(-6.0, 6.0, size=shape))
    raise ValueError(family)


def _weights(rng, nb, N1, family):
    if family == "exact":
        pick = np.argsort(rng.random((nb, N1, 4)), axis=2)[:, :, :3]
        return EXACT_WEIGHTS[pick]
    return rng.random((nb, N1, 3)) * 0.2 + np.array([0.2, 0.5, 0.8])


def ew_inputs(c, family="natural"):
    """The inputs of a group / gather / interp / backward case.  family "exact": integers up to 64 in magnitude and
    weights from {1/4, 1/2, 1, 2}: every product and every partial sum is exact in any order; "natural": normal values
    scaled by e^u, u uniform in [-6, 6]."""
    op, S, C, N, kind = c["op"], c["S"], c["C"], c["N"], c["kind"]
    rng = _rng(c, family == "exact")
    hot = kind == "hot"
    if op in ("group", "gather", "group_bwd"):
        M, K = mk_of(c)
        ix = make_index(rng, B, S, N, hot)
        ix = ix.reshape((B, M) if op == "gather" else (B, M, K))
        if op == "group_bwd":
            return dict(gout=_values(rng, (B, C, M, K), family), idx=ix)
        feat = _values(rng, (B, C, N), family)
        if kind == "nonfinite":
            feat[:, 0, 0], feat[:, 1, N - 1], feat[:, 2, 1] = np.nan, np.inf, -np.inf
        return dict(feat=feat, idx=ix)
    ix = make_index(rng, B, 3 * S, N, hot).reshape(B, S, 3)
    w = _weights(rng, B, S, family)
    if op == "interp_bwd":
        return dict(gout=_values(rng, (B, C, S), family), idx=ix, w=w)
    feat = _values(rng, (B, C, N), family)
    if kind == "nonfinite":
        feat[:, 0, 0], feat[:, 1, N - 1], feat[:, 2, 1] = np.nan, np.inf, -np.inf
        w[:, 5, :] = 0.0                              # inf 0 is NaN
    if kind == "signed_zero":
        feat[:, :, :] = -0.0                          # three products of -0.0: the reference's acc = 0 start gives +0.0
        feat[:, 1, 0] = 0.0
        feat[:, 2, N - 1] = -3.0
        w[:, 3, :] = 0.0                              # -3 0 = -0.0
    return dict(feat=feat, idx=ix, w=w)


def scene(inp, b):
    """Scene b of an input dict (or tuple) as its own B = 1 input."""
    if isinstance(inp, dict):
        return {k: v[b:b + 1] for k, v in inp.items()}
    return tuple(v[b:b + 1] if isinstance(v, np.ndarray) else v for v in inp)


def ew_model(c, inp, sab=None):
    op = c["op"]
    if op in ("group", "gather"):
        return group_points_np(inp["feat"], inp["idx"], sab)
    if op == "interp":
        return three_interpolate_np(inp["feat"], inp["idx"], inp["w"], c["fmad"], sab)
    if op == "group_bwd":
        return group_points_backward_np(inp["gout"], inp["idx"], c["N"], sab)
    return three_interpolate_backward_np(inp["gout"], inp["idx"], inp["w"], c["N"], sab)


def ew_oracle(O, c, inp):
    """The C oracle's double build on a case (inside oracle.double_dispatch())."""
    op = c["op"]
    if op == "gather":
        return O.gather_points(inp["feat"], inp["idx"])
    if op == "group":
        return O.group_points(inp["feat"], inp["idx"])
    if op == "interp":
        return O.three_interpolate(inp["feat"], inp["idx"], inp["w"], fmad=c["fmad"])
    if op == "group_bwd":
        return O.group_points_backward(inp["gout"], inp["idx"], c["N"])
    return O.three_interpolate_backward(inp["gout"], inp["idx"], inp["w"], c["N"])


def atomic_bound(c, inp):
    """gather_edges.atomic_bound for double -> (reference, bound), both (B, C, N) long double: per target
    n_j 2^-53 sum |terms_j|.  n_j contributions added in any order are within (n_j - 1) u sum |terms_j| of their exact
    sum, u = 2^-53, and the rounding of each product (interpolate) adds at most u |term|: n_j u sum |terms_j| to first
    order in u.  The reference is summed in long double (64-bit significand): its own error is 2^-11 of the bound."""
    nb = inp["idx"].shape[0]
    L = np.longdouble
    if c["op"] == "group_bwd":
        terms = inp["gout"].reshape(nb, c["C"], -1).astype(L)
    else:
        terms = (inp["gout"].astype(L)[:, :, :, None] * inp["w"].astype(L)[:, None, :, :]).reshape(nb, c["C"], -1)
    ix = inp["idx"].reshape(nb, -1)
    want, mag, count = (np.zeros((nb, c["C"], c["N"]), L) for _ in range(3))
    for b in range(nb):
        for ch in range(c["C"]):
            np.add.at(want[b, ch], ix[b], terms[b, ch])
            np.add.at(mag[b, ch], ix[b], np.abs(terms[b, ch]))
            np.add.at(count[b, ch], ix[b], L(1))
    return want, count * L(2.0 ** -53) * mag


def same(a, b):
    """Bit for bit, NaNs by position."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return bool(np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))
