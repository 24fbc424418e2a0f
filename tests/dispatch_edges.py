"""The dispatch ladder of the geometry operators: every size at which `launch_fps` (csrc/fps.hip), `bq_use_grid`
(csrc/ball_query.hip) and the 3-NN routing (functions.py, csrc/three_nn.hip) change the kernel they start, with its
neighbours.  Plain data plus the seeded inputs the cases run on: tests/test_dispatch_edges.py keeps the table honest
against the sources on the CPU (a moved threshold or a new kernel case fails there until this file follows),
tests/test_dispatch_edges_gpu.py runs every entry against the CPU oracle.

A per-lane-slot kernel goes wrong at the top of its range (every slot of every lane is full, nothing is padding) and
one past it (the last slot of the first lane holds exactly one real point): each threshold T is listed as T and
T + 1, and as T - 1 too.
"""
import numpy as np

# --------------------------------------------------------------------------------------------------------- FPS
# launch_fps picks by N, M, S4G_FPS_MODE and the workspace:
#   fps_reg_kernel<T, P>          N <= T P, first match of (256,1) (512,1) (512,2) (512,5) (512,10) (512,20) (512,32) (512,50)
#   fps_pruned_kernel<512, P>     P = 10 / 20 / 32 / 50 by the same N <= 512 P rule, where fps_use_pruned says so:
#                                 default N > 10 240, or N > 5 120 with M >= 2 048; mode "pruned" N > 2 560; mode "dense"
#                                 never; N <= 25 600 and M > FPS_PRUNED_MIN_PICKS (48) always
#   fps_pruned_l2_kernel<512, S>  25 600 < N <= 65 535, M >= 64, not mode "dense"; S = 100 up to FPS_L2_CAP (51 200), else 128
#   fps_stream_kernel             whatever is left
# One row per (N, mode); every M of the row with the kernel form it must reach.  The form's first word ("reg",
# "pruned", "l2", "stream") is what the GPU test can observe through the ABI; the template arguments say which
# instantiation the row is there for.
FPS_LADDER = [
    # ---- fps_reg_kernel, small sizes: M = N picks every point (all slots of all lanes are read as winners)
    (255, "default", ((255, "reg<256,1>"), (48, "reg<256,1>"))),
    (256, "default", ((256, "reg<256,1>"), (63, "reg<256,1>"))),
    (257, "default", ((257, "reg<512,1>"), (64, "reg<512,1>"))),
    (511, "default", ((511, "reg<512,1>"),)),
    (512, "default", ((512, "reg<512,1>"), (49, "reg<512,1>"))),
    (513, "default", ((513, "reg<512,2>"),)),
    (1023, "default", ((1023, "reg<512,2>"),)),
    (1024, "default", ((1024, "reg<512,2>"), (48, "reg<512,2>"))),
    (1025, "default", ((1025, "reg<512,5>"), (64, "reg<512,5>"))),
    (2559, "default", ((2559, "reg<512,5>"),)),
    (2560, "default", ((2560, "reg<512,5>"), (300, "reg<512,5>"))),
    (2560, "pruned", ((49, "reg<512,5>"), (300, "reg<512,5>"))),          # the forced-pruned rule is N > 2 560
    (2561, "default", ((2561, "reg<512,10>"), (49, "reg<512,10>"))),
    # ---- the smallest forced-pruned size; FPS_PRUNED_MIN_PICKS on both sides
    (2561, "pruned", ((47, "reg<512,10>"), (48, "reg<512,10>"), (49, "pruned<512,10>"), (300, "pruned<512,10>"),
                      (2561, "pruned<512,10>"))),
    (5119, "default", ((300, "reg<512,10>"),)),
    (5119, "pruned", ((300, "pruned<512,10>"),)),
    (5120, "default", ((300, "reg<512,10>"), (2048, "reg<512,10>"))),      # "N > 5 120 and M >= 2 048": not yet
    (5120, "dense", ((300, "reg<512,10>"),)),
    (5120, "pruned", ((48, "reg<512,10>"), (49, "pruned<512,10>"), (1024, "pruned<512,10>"))),
    # ---- the long-chain rule: M = 2 047 / 2 048 at both ends of (5 120, 10 240]
    (5121, "default", ((300, "reg<512,20>"), (2047, "reg<512,20>"), (2048, "pruned<512,20>"))),
    (5121, "pruned", ((48, "reg<512,20>"), (49, "pruned<512,20>"), (300, "pruned<512,20>"))),
    (10239, "default", ((2047, "reg<512,20>"), (2048, "pruned<512,20>"))),
    (10240, "default", ((300, "reg<512,20>"), (2047, "reg<512,20>"), (2048, "pruned<512,20>"), (2049, "pruned<512,20>"))),
    (10240, "dense", ((2048, "reg<512,20>"),)),
    (10240, "pruned", ((49, "pruned<512,20>"), (300, "pruned<512,20>"))),
    # ---- default-pruned from 10 241; the dense <512,32> and <512,50> forms at both ends
    (10241, "default", ((48, "reg<512,32>"), (49, "pruned<512,32>"), (300, "pruned<512,32>"))),
    (10241, "dense", ((300, "reg<512,32>"),)),
    (16383, "default", ((300, "pruned<512,32>"),)),
    (16384, "default", ((48, "reg<512,32>"), (49, "pruned<512,32>"), (2048, "pruned<512,32>"))),
    (16384, "dense", ((300, "reg<512,32>"),)),
    (16385, "default", ((48, "reg<512,50>"), (49, "pruned<512,50>"), (2100, "pruned<512,50>"))),
    (16385, "dense", ((300, "reg<512,50>"),)),
    (25599, "default", ((300, "pruned<512,50>"),)),
    (25600, "default", ((48, "reg<512,50>"), (49, "pruned<512,50>"), (2048, "pruned<512,50>"))),
    (25600, "dense", ((300, "reg<512,50>"),)),
    (25600, "pruned", ((300, "pruned<512,50>"),)),
    # ---- the L2-resident kernel: M = 63 / 64, 100 against 128 slots, the last size of the 16-bit positions
    (25601, "default", ((63, "stream"), (64, "l2<512,100>"), (400, "l2<512,100>"))),
    (25601, "dense", ((64, "stream"),)),
    (25601, "pruned", ((400, "l2<512,100>"),)),
    (51199, "default", ((400, "l2<512,100>"),)),
    (51200, "default", ((63, "stream"), (64, "l2<512,100>"), (2100, "l2<512,100>"))),
    (51201, "default", ((63, "stream"), (64, "l2<512,128>"), (400, "l2<512,128>"))),
    (65534, "default", ((400, "l2<512,128>"),)),
    (65535, "default", ((63, "stream"), (64, "l2<512,128>"), (400, "l2<512,128>"))),
    (65535, "dense", ((64, "stream"),)),
    (65536, "default", ((63, "stream"), (64, "stream"), (300, "stream"))),   # the L2 kernel must not be chosen
    (65537, "default", ((64, "stream"),)),
]

# one (N, M, mode) per kernel form for the fmad contract (S4G_FLAG_FMAD)
FPS_FMAD = [(256, 256, "default"), (512, 512, "default"), (1024, 1024, "default"), (2560, 300, "default"),
            (5120, 300, "default"), (10240, 300, "default"), (16384, 300, "dense"), (25600, 300, "dense"),
            (5120, 1024, "pruned"), (10240, 2048, "default"), (16384, 2048, "default"), (25600, 2048, "default"),
            (51200, 2100, "default"), (65535, 400, "default"), (65536, 64, "default")]

# pick distances (s4g_fps_gather_ex_i32's `dist`): both ends of the range of each form that reports them
FPS_PICK_DISTANCES = [(255, 255, "default"), (25600, 300, "dense"),            # reg
                      (2561, 300, "pruned"), (25600, 2048, "default"),         # pruned
                      (25601, 400, "default"), (65535, 400, "default")]        # pruned-L2

# workspace fallback: (N, M, mode, form with the full workspace, outcome with ws = NULL, outcome one byte short);
# an outcome is the form that must answer, or "EWORKSPACE"
FPS_WORKSPACE = [
    (16384, 300, "default", "pruned<512,32>", "reg<512,32>", "reg<512,32>"),
    (51201, 63, "default", "stream", "EWORKSPACE", "stream"),
    (51201, 400, "default", "l2<512,128>", "EWORKSPACE", "stream"),
]


# What s4g_workspace_bytes(S4G_OP_FPS) tells about a size: up to FPS_REG_TOP it is non-zero exactly where a pre-pass
# form may run (N above the mode's value here; never in mode "dense"); up to FPS_L2_TOP it holds the sort buffers
# (more than the streaming kernel's B N floats); past that it is exactly the streaming kernel's buffer.
FPS_MAY_PRUNE_ABOVE = {"default": 5120, "pruned": 2560}
FPS_REG_TOP, FPS_L2_TOP = 25600, 65535


def fps_cases():
    """[(N, M, mode, form)], one entry per collected GPU case."""
    return [(N, M, mode, form) for N, mode, ms in FPS_LADDER for M, form in ms]


def fps_form(N, M, mode, c):
    """launch_fps restated over the constants `c` the CPU test reads out of csrc/fps.hip (workspace present)."""
    def name(kind, cases):
        for T, P in cases:
            if N <= T * P:
                return "%s<%d,%d>" % (kind, T, P)
        return None
    top = max(T * P for T, P in c["reg"])
    if mode == "dense" or N > top:
        pruned = False
    elif mode == "pruned":
        pruned = N > c["forced_pruned_above"]
    else:
        pruned = N > c["pruned_above"] or (N > c["long_chain_above"] and M >= c["long_chain_picks"])
    if pruned and M > c["min_picks"] and name("pruned", c["pruned"]):
        return name("pruned", c["pruned"])
    if name("reg", c["reg"]):
        return name("reg", c["reg"])
    if mode != "dense" and N <= c["l2_cap_big"] and M >= c["l2_min_picks"]:
        return "l2<512,%d>" % (100 if N <= c["l2_cap"] else 128)
    return "stream"


# --------------------------------------------------------------------------------------------------------- ball query
# bq_use_grid: N > GR_MAX_POINTS (65 536) or K > 1 024 -> scan; S4G_BQ_MODE=grid -> grid; auto -> grid from N >= 8 192
BQ_N = [8191, 8192, 8193, 65535, 65536, 65537]
BQ_K = [1, 64, 1023, 1024, 1025]
BQ_M = 301            # not a multiple of 4: the last workgroup's four waves are not all busy
BQ_GRID_MIN_N, BQ_GRID_MAX_N, BQ_GRID_MAX_K = 8192, 65536, 1024


def bq_cases():
    """[(N, K, mode, path)]: auto everywhere, S4G_BQ_MODE=grid wherever the grid is legal."""
    out = []
    for N in BQ_N:
        for K in BQ_K:
            legal = N <= BQ_GRID_MAX_N and K <= BQ_GRID_MAX_K
            out.append((N, K, "auto", "grid" if legal and N >= BQ_GRID_MIN_N else "scan"))
            if legal:
                out.append((N, K, "grid", "grid"))
    return out


# --------------------------------------------------------------------------------------------------------- 3-NN
# functions.py: the cell grid for 2 048 <= N2 <= GR_MAX_POINTS (unless S4G_NN_MODE=scan), else the scan entry;
# launch_three_nn_scan: the split scan for 24 <= N2 <= 2 048 (unless S4G_NN_SPLIT=0), 4 lanes per query below
# 256 keys and 8 from there on; launch_three_nn_grid refuses N2 > GR_MAX_POINTS.  25, 257 and 2 041 leave the
# split scan's last round with ONE key (N2 mod S == 1).
NN_N2 = [3, 4, 5, 23, 24, 25, 255, 256, 257, 2041, 2047, 2048, 2049, 65535, 65536, 65537]
NN_N1 = 1001          # not a multiple of 256: the last workgroup is ragged
NN_SPLIT_MIN, NN_SPLIT_WIDE, NN_SPLIT_MAX = 24, 256, 2048
NN_GRID_MIN, NN_GRID_MAX = 2048, 65536
NN_GRID_ENTRY_N2 = [3, 4, 2047, 65535, 65536]      # the grid entry called directly (legal for 3 <= N2 <= GR_MAX_POINTS)


def nn_cases():
    """[(N2, knob, value, path)] through the operator API: default everywhere, plus the other side of the knob that
    decides at that size (S4G_NN_SPLIT=0 in the split range, S4G_NN_MODE=scan in the grid range)."""
    out = []
    for N2 in NN_N2:
        grid = NN_GRID_MIN <= N2 <= NN_GRID_MAX
        split = NN_SPLIT_MIN <= N2 <= NN_SPLIT_MAX
        out.append((N2, None, None, "grid" if grid else "split" if split else "scan"))
        if grid:
            out.append((N2, "S4G_NN_MODE", "scan", "split" if split else "scan"))
        if split:
            out.append((N2, "S4G_NN_SPLIT", "0", "grid" if grid else "scan"))
    return out


# --------------------------------------------------------------------------------------------------------- inputs
def seed_of(*key):
    return int(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def uniform_cloud(seed, B, N):
    return np.random.default_rng(seed).random((B, 3, N), dtype=np.float32)


def lattice_levels(N):
    """Lattice steps per axis for N points: about N / 3 distinct positions, so points coincide AND distinct points sit at
    equal distances (levels ** 3 < N for every N >= 36: fewer positions than points)."""
    return max(4, int(np.ceil((N / 3.0) ** (1.0 / 3.0))))


def lattice_cloud(seed, B, N):
    """test_ops_gpu._quantized on a 2^-5 lattice: every coordinate, difference and squared distance is exact in
    fp32, so equal distances are equal bit for bit and the tie rule decides the picks."""
    from tests.test_ops_gpu import _quantized
    return _quantized(np.random.default_rng(seed), B, N, levels=lattice_levels(N), scale=0.03125)


def distinct_points(cloud_3n):
    return len(np.unique(np.ascontiguousarray(cloud_3n.T), axis=0))


def fps_inputs(N, M):
    """{kind: (2, 3, N) float32}: B = 2 different scenes of uniform random points and of the tie-heavy lattice; above
    10 240 points one table-top batch as well."""
    out = {"uniform": uniform_cloud(seed_of(N, M, 1), 2, N), "lattice": lattice_cloud(seed_of(N, M, 2), 2, N)}
    if N > 10240:
        from s4g_release_amd import synth
        out["tabletop"] = synth.make_batch([N % 7, 7 + M % 11], N)
    return out


def prefix_steps(M):
    """M2 of the prefix check over a level of M picks."""
    return max(2, M // 2)


def bq_radius(N, K):
    """A radius for which the table-top scene has short and full balls: 40 % of the points lie on the 0.62 m x 0.60 m
    table, so a disc around an interior table point holds about 1.3 max(K, 8) of them (full; more on the objects),
    and one around a point on the table's rim a half or a quarter of that (short)."""
    return float(np.float32(np.sqrt(1.3 * max(K, 8) / (np.pi * (0.40 / (0.62 * 0.60)) * N))))


def bq_inputs(N, K):
    """(points (2, 3, N), centroids (2, 3, BQ_M), radius): centroids are points of the scene, three per scene moved
    5 m away (empty balls)."""
    from s4g_release_amd import synth
    pts = synth.make_batch([1, 4], N)
    rng = np.random.default_rng(seed_of(N, K, 3))
    ctr = np.stack([pts[b][:, rng.choice(N, BQ_M, replace=False)] for b in range(2)]).astype(np.float32)
    ctr[:, 0, :3] += np.float32(5.0)
    return pts, np.ascontiguousarray(ctr), bq_radius(N, K)


def bq_has_all_ball_kinds(cnt, K):
    """Empty, full and (K > 1: a ball of one neighbour slot is empty or full) short balls in every scene."""
    return all((c == 0).any() and (c == K).any() and (K == 1 or ((c > 0) & (c < K)).any()) for c in cnt)


def nn_inputs(N2):
    """{kind: (queries (2, 3, NN_N1), keys (2, 3, N2))}.  "tabletop": keys are points of one table-top batch, queries
    those of another over the same table, three of them copies of keys (distance 0) and three far from every key;
    "lattice": both on one coarse lattice, so nearly every query has equidistant keys and the earlier index wins."""
    from s4g_release_amd import synth
    keys = synth.make_batch([0, 7], max(N2, 64))[:, :, :N2]
    q = synth.make_batch([3, 5], NN_N1)
    q[:, :, :3] = keys[:, :, :3]
    q[:, :, 3:6] += np.float32(5.0)
    rng = np.random.default_rng(seed_of(N2, 5))
    levels = lattice_levels(max(N2, 192))
    lat = rng.integers(0, levels, size=(2, 3, NN_N1 + N2)).astype(np.float32) * np.float32(0.03125)
    return {"tabletop": (np.ascontiguousarray(q), np.ascontiguousarray(keys)),
            "lattice": (np.ascontiguousarray(lat[:, :, :NN_N1]), np.ascontiguousarray(lat[:, :, NN_N1:]))}


# --------------------------------------------------------------------------------------------------------- arithmetic
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 arrays (numpy has no fused multiply-add).  The product of two
    24-bit significands is exact in float64; the sum is rounded to odd there (the error term of TwoSum says on which
    side of the rounded sum the exact one lies), and a round-to-odd result with 53 >= 2 * 24 + 2 bits rounds to
    float32 like the exact sum."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c, p.shape).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even & np.isfinite(s), odd, s).astype(np.float32)


def dist2(c_31, p_3n, fmad=False):
    """Squared distances centroid -> points under the distance contract of include/s4g_ops.h, every operation rounded
    to fp32: strict ((dx dx) + (dy dy)) + (dz dz); fmad fma(dz, dz, fma(dy, dy, dx dx))."""
    d = p_3n.astype(np.float32) - c_31.astype(np.float32)
    if fmad:
        return fma32(d[2], d[2], fma32(d[1], d[1], d[0] * d[0]))
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def pick_distances(pts_3n, idx_m, fmad=False):
    """D_k, k >= 1: the running minimum squared distance pick k had when it was taken (+inf for pick 0)."""
    c = pts_3n[:, idx_m].astype(np.float32)
    M = c.shape[1]
    out = np.full(M, np.inf, np.float32)
    md = np.full(M, np.inf, np.float32)
    for k in range(1, M):
        md = np.minimum(md, dist2(c[:, k - 1:k], c, fmad))
        out[k] = md[k]
    return out


def prefix_is_proven(ctr_3m, dist_m, M2, fmad=False):
    """fps_prefix_check_kernel restated: True iff at every step k < M2 element k's own running min-distance is the
    reported D_k, positive and finite, and every later element stays strictly below it."""
    M1 = ctr_3m.shape[1]
    md = np.full(M1, np.inf, np.float32)
    for k in range(1, M2):
        md = np.minimum(md, dist2(ctr_3m[:, k - 1:k], ctr_3m, fmad))
        D = dist_m[k]
        if not (D > 0 and np.isfinite(D)) or md[k].tobytes() != np.float32(D).tobytes() or (md[k + 1:] >= D).any():
            return False
    return True
