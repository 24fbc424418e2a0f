"""The data-movement operators at their edges: group_points / gather_points (csrc/group.hip), three_interpolate, its
channels-last forms and interp_add_cl (csrc/interpolate.hip), and both backwards, atomic and deterministic
(csrc/scatter.hip).  Plain data and numpy: one case table per C entry point with every kernel constant T as T - 1, T,
T + 1 on the axis it bounds, the seeded inputs the cases run on, numpy restatements of every operator, and sabotaged
variants of those restatements.  tests/test_gather_edges.py keeps the tables honest against the sources on the CPU and
shows that the inputs see every sabotage; tests/test_gather_edges_gpu.py runs every case through the C ABI into guarded
buffers.

A case is a dict: "op" names the entry point, the sizes follow, "ws" says what workspace the call is handed ("full",
"null", "short", "misaligned"), "mis" which pointers are offset on purpose and by how many bytes, "mode" the value of
S4G_INTERP_MODE.  `form(case)` restates the C entry point's choice of kernel."""
import itertools

import numpy as np

from tests.dispatch_edges import fma32, seed_of

# ------------------------------------------------------------------------------------------------------ constants
# (tests/test_gather_edges.py reads each of them out of the sources and fails when one moves)
GP_THREADS, GP_CG = 256, 8                      # csrc/group.hip: lanes (x 4 slots in the vec4 form), channels per block row
IP_THREADS, IP_CG, IPQ = 256, 16, 32            # csrc/interpolate.hip: lanes, channels per block row, quads per block row
IPT_PTS, IPT_CH, CL_TILE = 64, 64, 32           # the 64 x 64 tile kernels; feat_to_channels_last's 32 x 32 tile
IA_ROWS, IA_THREADS, IA_MAX_C = 8, 256, 1024    # interp_add_cl
SC_THREADS, SC_TILE, SC_CL_MIN_C = 256, 64, 32  # csrc/scatter.hip
RS_TILE = 2048                                  # csrc/radix_sort.hip: elements per workgroup of the sort
XCDS = 8                                        # the tile kernels round their slice count up to this
ROUTE_MIN_MK, ROUTE_MIN_C = 4096, 16            # functions.py

GROUP_OPS = ("group", "gather", "group_xyz", "group_ws")
INTERP_OPS = ("interp", "interp_ws")
BWD_OPS = ("group_bwd", "interp_bwd")


def _mk(MK):
    """(M, K) with M K = MK."""
    for K in (4, 3, 2):
        if MK % K == 0:
            return MK // K, K
    return MK, 1


def _unique(cases):
    """The cases without repeats, in their order (two ladders may meet in one shape)."""
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return out


def _group(op, B, C, N, MK, ws=None, mis=None):
    M, K = (MK, 1) if op == "gather" else _mk(MK)
    return dict(op=op, B=B, C=3 if op == "group_xyz" else C, N=N, M=M, K=K, ws=ws, mis=mis or {})


def _interp(op, B, C, N2, N1, fmad, ws=None, mis=None, mode=None):
    return dict(op=op, B=B, C=C, N2=N2, N1=N1, fmad=fmad, ws=ws, mis=mis or {}, mode=mode)


# ------------------------------------------------------------------------------------------------------ grouping
GROUP_VEC4_MK = [4, 4 * GP_THREADS - 4, 4 * GP_THREADS, 4 * GP_THREADS + 4]           # 4, 1020, 1024, 1028
GROUP_VEC4_C = [1, GP_CG - 1, GP_CG, GP_CG + 1, 2 * GP_CG + 1]
GROUP_SCALAR_MK = [1, 3, 5, GP_THREADS - 1, GP_THREADS, GP_THREADS + 1, 4 * GP_THREADS - 1]
GATHER_M = [1, GP_THREADS - 1, GP_THREADS, GP_THREADS + 1]
GROUP_XYZ_MK = GROUP_VEC4_MK
GROUP_XYZ_N = [1, GP_THREADS - 1, GP_THREADS, GP_THREADS + 1]
TILE_S = [1, 3, 4, IPT_PTS - 1, IPT_PTS, IPT_PTS + 1, IPT_PTS + 2, 2 * IPT_PTS - 1, 2 * IPT_PTS, 2 * IPT_PTS + 1]
TILE_C = [4, IPT_CH - 4, IPT_CH, IPT_CH + 4, 2 * IPT_CH + 4]
TILE_N = [1, CL_TILE - 1, CL_TILE, CL_TILE + 1]
TILE_SLICES = [(1, 64), (7, 60), (8, 64), (4, 68), (9, 64), (3, 132), (17, 4)]       # (B, C): B ceil(C / 64) = 1, 7, 8, 8, 9, 9, 17


def group_cases():
    out = []
    for MK, C, B in itertools.product(GROUP_VEC4_MK, GROUP_VEC4_C, (1, 3)):
        out.append(_group("group", B, C, 37, MK))
    for MK, C in itertools.product(GROUP_SCALAR_MK, (1, GP_CG + 1)):
        # (a multiple of 4 is the vec4 form's: the scalar kernel sees it through an output that is off by one word)
        out.append(_group("group", 3, C, 37, MK, mis={"out": 4} if MK % 4 == 0 else None))
    out.append(_group("group", 3, 9, 37, 1024, mis={"idx": 8}))
    out.append(_group("group", 3, 9, 37, 1024, mis={"out": 4}))
    for M in GATHER_M:
        out.append(_group("gather", 3, 9, 37, M))
    for MK, N in itertools.product(GROUP_XYZ_MK, GROUP_XYZ_N):
        out.append(_group("group_xyz", 3, 3, N, MK, ws="full"))
    for ws, mis, MK in (("null", {}, 1024), ("short", {}, 1024), ("misaligned", {}, 1024), ("full", {"idx": 8}, 1024),
                        ("full", {"out": 4}, 1024), ("full", {}, 1022)):
        out.append(_group("group_xyz", 3, 3, 257, MK, ws=ws, mis=mis))
    for S in TILE_S:
        out.append(_group("group_ws", 2, 68, 33, S, ws="full"))
    for C, S in itertools.product(TILE_C, (IPT_PTS, IPT_PTS + 1, IPT_PTS + 2)):
        out.append(_group("group_ws", 2, C, 33, S, ws="full"))
    for N in TILE_N:
        out.append(_group("group_ws", 2, 68, N, 66, ws="full"))
    for B, C in TILE_SLICES:
        out.append(_group("group_ws", B, C, 33, 65, ws="full"))
        out.append(_group("group_ws", B, C, 33, 128, ws="full"))
    out.append(_group("group_ws", 2, 6, 33, 64, ws="full"))
    out.append(_group("group_ws", 2, 68, 33, 64, ws="short"))
    out.append(_group("group_ws", 2, 68, 33, 64, ws="null"))
    out.append(_group("group_ws", 2, 68, 33, 64, ws="misaligned"))
    out.append(_group("group_ws", 2, 68, 33, 64, ws="full", mis={"out": 4}))
    return _unique(out)


# ------------------------------------------------------------------------------------------------------ interpolation
INTERP_N1 = [1, IP_THREADS - 1, IP_THREADS, IP_THREADS + 1]
INTERP_C = [1, IP_CG - 1, IP_CG, IP_CG + 1, 2 * IP_CG + 1]
INTERP_N2 = [1, 3]
LANE_C = [4, 4 * IPQ - 4, 4 * IPQ, 4 * IPQ + 4, 8 * IPQ + 4]                          # 4, 124, 128, 132, 260


def interp_cases():
    out = []
    for N1, C, N2, fmad in itertools.product(INTERP_N1, INTERP_C, INTERP_N2, (0, 1)):
        out.append(_interp("interp", 2, C, N2, N1, fmad))
    for fmad in (0, 1):
        for S in TILE_S:
            out.append(_interp("interp_ws", 2, 68, 33, S, fmad, ws="full"))
        for C, S in itertools.product(TILE_C, (IPT_PTS, IPT_PTS + 1, IPT_PTS + 2)):
            out.append(_interp("interp_ws", 2, C, 33, S, fmad, ws="full"))
        for N2 in TILE_N:
            out.append(_interp("interp_ws", 2, 68, N2, 66, fmad, ws="full"))
        for B, C in TILE_SLICES:
            out.append(_interp("interp_ws", B, C, 33, 65, fmad, ws="full"))
            out.append(_interp("interp_ws", B, C, 33, 128, fmad, ws="full"))
        for C, N1 in itertools.product(LANE_C, INTERP_N1):
            out.append(_interp("interp_ws", 2, C, 33, N1, fmad, ws="full", mode="lane"))
        out.append(_interp("interp_ws", 2, 132, 33, 257, fmad, ws="full", mis={"out": 4}))      # the lane form without the knob
        out.append(_interp("interp_ws", 2, 132, 33, 256, fmad, ws="full", mis={"out": 8}))
        out.append(_interp("interp_ws", 2, 6, 33, 65, fmad, ws="full"))
        for ws in ("null", "short", "misaligned"):
            out.append(_interp("interp_ws", 2, 68, 33, 65, fmad, ws=ws))
    return _unique(out)


def form(c):
    """The kernel the C entry point starts for a case, restated from csrc/group.hip and csrc/interpolate.hip."""
    op, mis, ws = c["op"], c["mis"], c["ws"]
    ws_ok = ws == "full"
    if op in GROUP_OPS:
        MK = c["M"] * c["K"]
        plain = "vec4" if MK % 4 == 0 and not mis.get("idx", 0) % 16 and not mis.get("out", 0) % 16 else "scalar"
        if op == "group_xyz" and ws_ok and plain == "vec4":
            return "aos"
        if op == "group_ws" and ws_ok and c["C"] % 4 == 0 and not mis.get("out", 0) % 16:
            return "tile"
        return plain
    if op == "interp_ws" and ws_ok and c["C"] % 4 == 0:
        return "tile" if c["mode"] != "lane" and not mis.get("out", 0) % 16 else "lane"
    return "plain"


# ------------------------------------------------------------------------------------------------------ interp_add_cl
IA_C = [4, 8, 12, 252, 256, 260, 512, 516, 1020, 1024]      # C / 4 = 1, 2, 3, 63, 64, 65, 128, 129, 255, 256
IA_REFUSED_C = [IA_MAX_C + 4, 6]


def ia_rows_per_block(C):
    """R: the rows one workgroup of interp_add_cl_kernel handles."""
    return IA_ROWS * (IA_THREADS // (C // 4))


def interp_add_shapes():
    """[(B, N1, C)]: B N1 = 1, R - 1, R, R + 1 in one scene; three scenes of R, 2 R and of R + 1 rows."""
    out = []
    for C in IA_C:
        R = ia_rows_per_block(C)
        for N1 in (1, R - 1, R, R + 1):
            if N1 >= 1 and (1, N1, C) not in out:
                out.append((1, N1, C))
        out += [(3, R, C), (3, R + 1, C)]
        if C >= 252:
            out.append((3, 2 * R, C))
    return out


def interp_add_cases():
    out = []
    for (B, N1, C), y, relu, amax in itertools.product(interp_add_shapes(), (0, 1), (0, 1), (0, 1)):
        out.append(dict(op="interp_add", B=B, N1=N1, N2=5, C=C, y=y, relu=relu, amax=amax))
    return out


# ------------------------------------------------------------------------------------------------------ backward
BWD_C = [1, SC_CL_MIN_C - 1, SC_CL_MIN_C, SC_CL_MIN_C + 1, SC_TILE - 1, SC_TILE, SC_TILE + 1]
BWD_N = [1, SC_TILE - 1, SC_TILE, SC_TILE + 1, SC_THREADS - 1, SC_THREADS, SC_THREADS + 1]
BWD_T = [1, SC_TILE - 1, SC_TILE, SC_TILE + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1]
BWD_N1 = [1, 21, 22, 63, 64, 65, 683]            # T = 3 N1 = 3, 63, 66, 189, 192, 195, 2049
BWD_KEY_WIDTH = [(3, 21845), (2, 32768)]         # B N = 65 535 (16 key bits, two sort passes) and 65 536 (17, three)
# the atomic kernels' own launch shapes: channels per block row, and one lane per position (MK) / per dense point (N1)
BWD_ATOMIC_C = {"group_bwd": [GP_CG - 1, GP_CG, GP_CG + 1], "interp_bwd": [IP_CG - 1, IP_CG, IP_CG + 1]}
BWD_ATOMIC_S = {"group_bwd": [GP_THREADS - 1, GP_THREADS, GP_THREADS + 1],
                "interp_bwd": [IP_THREADS - 1, IP_THREADS, IP_THREADS + 1]}


def _bwd(op, B, C, N, S, oob=0):
    if op == "group_bwd":
        M, K = _mk(S)
        return dict(op=op, B=B, C=C, N=N, M=M, K=K, oob=oob)
    return dict(op=op, B=B, C=C, N=N, N1=S, oob=oob)


def bwd_cases():
    out = []
    for op, sizes in (("group_bwd", BWD_T), ("interp_bwd", BWD_N1)):
        mid = sizes[3]
        for C in BWD_C:
            out.append(_bwd(op, 2, C, 65, mid))
            out.append(_bwd(op, 2, C, 65, mid, oob=1))
        for N in BWD_N:                                       # B = 1: B N = 255, 256, 257 among them
            for C in (1, SC_CL_MIN_C + 1):
                out.append(_bwd(op, 1, C, N, mid))
                out.append(_bwd(op, 1, C, N, mid, oob=1))
        for S in sizes:
            for C in (1, SC_CL_MIN_C):
                out.append(_bwd(op, 2, C, 64, S))
                if S >= 22:
                    out.append(_bwd(op, 2, C, 64, S, oob=1))
        for B, N in BWD_KEY_WIDTH:
            out.append(_bwd(op, B, 2, N, mid, oob=1))
            out.append(_bwd(op, B, SC_CL_MIN_C, N, mid))
        for C in BWD_ATOMIC_C[op]:
            out.append(_bwd(op, 2, C, 65, mid))
        for S in BWD_ATOMIC_S[op]:
            out.append(_bwd(op, 2, BWD_ATOMIC_C[op][2], 64, S))
        out.append(_bwd(op, 2, 33, 65, 0))                    # T = 0: exact zeros
    return out


def bwd_T(c):
    return c["M"] * c["K"] if c["op"] == "group_bwd" else 3 * c["N1"]


# ------------------------------------------------------------------------------------------------------ Python routing
ROUTE_GROUP_MK = [ROUTE_MIN_MK - 4, ROUTE_MIN_MK - 1, ROUTE_MIN_MK, ROUTE_MIN_MK + 1, ROUTE_MIN_MK + 4]
ROUTE_GROUP_C = [3, 4, ROUTE_MIN_C - 4, ROUTE_MIN_C - 1, ROUTE_MIN_C, ROUTE_MIN_C + 1, ROUTE_MIN_C + 4]
ROUTE_INTERP_C = ROUTE_GROUP_C[2:]
ROUTE_N2 = 100
ROUTE_INTERP_N1 = [ROUTE_N2 - 1, ROUTE_N2, ROUTE_N2 + 1]


def group_route(B, C, MK, min_mk=ROUTE_MIN_MK, min_c=ROUTE_MIN_C):
    """functions._group_points_forward's choice of entry point."""
    if C == 3 and B > 0 and MK % 4 == 0 and MK >= min_mk:
        return "s4g_group_points_xyz_f32"
    if C % 4 == 0 and C >= min_c and B > 0 and MK >= min_mk:
        return "s4g_group_points_ws_f32"
    return "s4g_group_points_f32"


def interp_route(B, C, N2, N1, min_c=ROUTE_MIN_C):
    """functions._interpolate_forward's choice of entry point."""
    if C % 4 == 0 and C >= min_c and B * N1 > 0 and N1 >= N2:
        return "s4g_three_interpolate_ws_f32"
    return "s4g_three_interpolate_f32"


def route_cases():
    out = []
    for MK, C in itertools.product(ROUTE_GROUP_MK, ROUTE_GROUP_C):
        M, K = _mk(MK)
        out.append(dict(op="route_group", B=2, C=C, N=50, M=M, K=K, entry=group_route(2, C, MK)))
    out.append(dict(op="route_group", B=0, C=16, N=50, M=1024, K=4, entry=group_route(0, 16, 4096)))
    for C, N1 in itertools.product(ROUTE_INTERP_C, ROUTE_INTERP_N1):
        out.append(dict(op="route_interp", B=2, C=C, N2=ROUTE_N2, N1=N1, fmad=0,
                        entry=interp_route(2, C, ROUTE_N2, N1)))
    out.append(dict(op="route_interp", B=0, C=16, N2=ROUTE_N2, N1=ROUTE_N2, fmad=0,
                    entry=interp_route(0, 16, ROUTE_N2, ROUTE_N2)))
    return out


def all_cases():
    return group_cases() + interp_cases() + interp_add_cases() + bwd_cases() + route_cases()


def case_id(c):
    parts = [c["op"]]
    for k in ("B", "C", "N", "N2", "M", "K", "N1"):
        if k in c:
            parts.append("%s=%d" % (k, c[k]))
    for k in ("fmad", "y", "relu", "amax", "oob"):
        if c.get(k):
            parts.append(k)
    if c.get("ws") and c["ws"] != "full":
        parts.append("ws-" + c["ws"])
    if c.get("mode"):
        parts.append(c["mode"])
    for k, v in sorted(c.get("mis", {}).items()):
        parts.append("%s+%d" % (k, v))
    return "-".join(parts)


# ------------------------------------------------------------------------------------------------------ inputs
EXACT_WEIGHTS = np.float32([0.25, 0.5, 1.0, 2.0])
EXACT_MAX = 64


def make_index(rng, B, T, N):
    """(B, T) int64 in [0, N): every scene holds 0 and N - 1 (one of them where T == 1), in an order that alternates from
    scene to scene; the last slot differs from the one before it (N > 1)."""
    ix = rng.integers(0, N, size=(B, T), dtype=np.int64)
    for b in range(B):
        ends = (0, N - 1) if b % 2 == 0 else (N - 1, 0)
        if T >= 1:
            ix[b, 0] = ends[0]
        if T >= 2:
            ix[b, 1] = ends[1]
        if T >= 3:
            ix[b, T - 1] = (ix[b, T - 2] + 1 + b) % N
    return ix


def oob_positions(T):
    """{position: what to put there} of the deterministic backward's out-of-range indices ("N" stands for the size)."""
    out = {}
    if T >= 5:
        out[2] = -3
        out[3] = "N"
    if T >= 8:
        out[T // 2] = 2 ** 40
    return out


def _values(rng, shape, family):
    if family == "exact":
        return rng.integers(-EXACT_MAX, EXACT_MAX + 1, size=shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _weights(rng, B, N1, family):
    """(B, N1, 3) float32, the three of a point distinct."""
    if family == "exact":
        pick = np.argsort(rng.random((B, N1, 4)), axis=2)[:, :, :3]
        return EXACT_WEIGHTS[pick]
    return (rng.random((B, N1, 3)) * 0.2 + np.array([0.2, 0.5, 0.8])).astype(np.float32)


def inputs(c, family="normal"):
    """The seeded numpy inputs of a case.  family "normal": i.i.d. normal features and gradients, weights in
    (0.2, 1.0); "exact": integer features and gradients up to 64 in magnitude and weights from {1/4, 1/2, 1, 2}, so that
    every product and every partial sum is exact in fp32 in any order."""
    op = c["op"]
    rng = np.random.default_rng(seed_of(*(int(v) for k, v in sorted(c.items()) if isinstance(v, (int, np.integer))),
                                        len(op), family == "exact"))
    B = c["B"]
    if op in GROUP_OPS or op == "route_group":
        M, K = c["M"], c["K"]
        ix = make_index(rng, B, M * K, c["N"])
        return dict(feat=_values(rng, (B, c["C"], c["N"]), family), idx=ix.reshape((B, M) if op == "gather" else (B, M, K)))
    if op in INTERP_OPS or op == "route_interp":
        ix = make_index(rng, B, 3 * c["N1"], c["N2"]).reshape(B, c["N1"], 3)
        return dict(feat=_values(rng, (B, c["C"], c["N2"]), family), idx=ix, w=_weights(rng, B, c["N1"], family))
    if op == "interp_add":
        N1, N2, C = c["N1"], c["N2"], c["C"]
        ix = make_index(rng, B, 3 * N1, N2).reshape(B, N1, 3).astype(np.int32)
        return dict(sp=_values(rng, (B * N2, C), family), idx=ix, w=_weights(rng, B, N1, family),
                    bias=_values(rng, (C,), family), y=_values(rng, (B * N1, C), family) if c["y"] else None)
    T = bwd_T(c)
    ix = make_index(rng, B, T, c["N"])
    if c["oob"]:
        for pos, v in oob_positions(T).items():
            ix[:, pos] = c["N"] if v == "N" else v
    if op == "group_bwd":
        return dict(gout=_values(rng, (B, c["C"], c["M"], c["K"]), family), idx=ix.reshape(B, c["M"], c["K"]))
    return dict(gout=_values(rng, (B, c["C"], c["N1"]), family), idx=ix.reshape(B, c["N1"], 3),
                w=_weights(rng, B, c["N1"], family))


def in_range_twin(c, inp):
    """The inputs of a backward case with every out-of-range position made a no-op the oracle accepts: index 0 with
    a zero gradient (group_points) or a zero weight (three_interpolate).  acc + 0 is acc, so the sums do not move."""
    N = c["N"]
    ix = inp["idx"]
    bad = (ix < 0) | (ix >= N)
    out = dict(inp, idx=np.where(bad, 0, ix))
    if c["op"] == "group_bwd":
        out["gout"] = np.where(bad[:, None], np.float32(0), inp["gout"])
    else:
        out["w"] = np.where(bad, np.float32(0), inp["w"])
    return out


# ------------------------------------------------------------------------------------------------------ restatements
NOT_WRITTEN = np.float32(np.nan)      # what a sabotaged restatement leaves where the kernel would not have stored

SABOTAGES = {
    # name: (ops it applies to, what goes wrong)
    "scene_base": (GROUP_OPS + INTERP_OPS + BWD_OPS + ("interp_add",), "the scene base of the index (b MK, b N1 3, b N2) dropped"),
    "idx_t1": (GROUP_OPS + INTERP_OPS + BWD_OPS + ("interp_add",), "the index read at t + 1"),
    "last_quad": (GROUP_OPS + INTERP_OPS, "the last quad of MK / N1 not written"),
    "cg_tail": (("group", "gather", "group_xyz"), "the channel-group tail ch >= 8 floor(C / 8) not written"),
    "last_slice": (("group_ws", "interp_ws"), "the last (scene, 64-channel) slice not written"),
    "weights_rotated": (INTERP_OPS + ("interp_bwd", "interp_add"), "the three neighbours' weights rotated"),
    "vec_rows_tail": (("group_ws", "interp_ws"), "rows N1 - N1 % 4 .. stored by the vector path: 16 bytes into the next row"),
    "bias_before_y": (("interp_add",), "(acc + bias) + y instead of (y + acc) + bias"),
    "relu_always": (("interp_add",), "ReLU applied with relu = 0"),
    "sentinel_first": (BWD_OPS, "the sentinel key sorted first: out-of-range positions land in target 0"),
    "descending": (BWD_OPS, "a target's contributions summed in descending position"),
    "cl_swapped": (("group_ws", "interp_ws"), "the channels-last copy's bounds test with C and S swapped on a ragged tile"),
    "k_stride": (INTERP_OPS + ("interp_add",), "neighbour k read with stride 1 from slot n instead of 3 n + k"),
}


def _shift(a):
    flat = a.reshape(-1)
    return np.concatenate([flat[1:], flat[:1]]).reshape(a.shape)


def _cl_copy(feat, sab):
    """(B, C, N) -> (B, N, C), feat_to_channels_last_kernel."""
    B, C, N = feat.shape
    out = np.ascontiguousarray(feat.transpose(0, 2, 1))
    if sab == "cl_swapped":
        cc, nn = np.meshgrid(np.arange(C), np.arange(N))                       # (N, C)
        ragged = ((C % CL_TILE != 0) & (cc // CL_TILE == (C - 1) // CL_TILE)) | \
                 ((N % CL_TILE != 0) & (nn // CL_TILE == (N - 1) // CL_TILE))
        out[:, ragged & ~((cc < N) & (nn < C))] = NOT_WRITTEN
    return out


def _store_sabotage(out, sab, cg):
    """`out` (B, C, S) after a kernel whose stores go wrong in the way `sab` names."""
    B, C, S = out.shape
    if sab == "last_quad":
        out[:, :, 4 * ((S - 1) // 4):] = NOT_WRITTEN
    elif sab == "cg_tail":
        out[:, cg * (C // cg):, :] = NOT_WRITTEN
    elif sab == "last_slice":
        out[B - 1, IPT_CH * ((C - 1) // IPT_CH):, :] = NOT_WRITTEN
    elif sab == "vec_rows_tail" and S % 4:
        flat = out.reshape(-1)
        for r in range(1, B * C):
            flat[r * S:r * S + min(4 - S % 4, S)] = NOT_WRITTEN
    return out


def group_points_np(feat, idx, sab=None):
    """out[b, c, t] = feat[b, c, idx[b, t]]; `idx` (B, M, K) or (B, M)."""
    B, C, N = feat.shape
    ix = idx.reshape(B, int(np.prod(idx.shape[1:])))
    if sab == "scene_base":
        ix = np.broadcast_to(ix[:1], ix.shape)
    elif sab == "idx_t1":
        ix = _shift(ix)
    src = _cl_copy(feat, sab).transpose(0, 2, 1) if sab == "cl_swapped" else feat
    out = np.take_along_axis(src, np.broadcast_to(ix[:, None, :], (B, C, ix.shape[1])), axis=2).copy()
    return _store_sabotage(out, sab, GP_CG).reshape((B, C) + idx.shape[1:])


def _neighbours(idx, w, sab):
    """The (index, weight) streams a kernel with the wiring error `sab` reads."""
    if sab == "scene_base":
        return np.broadcast_to(idx[:1], idx.shape), np.broadcast_to(w[:1], w.shape)
    if sab == "idx_t1":
        return _shift(idx), w
    if sab == "weights_rotated":
        return idx, np.roll(w, 1, axis=2)
    if sab == "k_stride":
        B, N1, _ = idx.shape
        fi, fw = idx.reshape(B, -1), w.reshape(B, -1)
        at = np.minimum(np.arange(N1)[:, None] + np.arange(3)[None, :], 3 * N1 - 1)
        return fi[:, at], fw[:, at]
    return idx, w


def three_interpolate_np(feat, idx, w, fmad=0, sab=None, f64=False):
    """acc = 0; acc += feat[b, c, idx[b, n, k]] * w[b, n, k] for k = 0, 1, 2: every product and sum rounded to fp32
    (strict), an fma chain (fmad), or all of it in float64."""
    B, C, N2 = feat.shape
    N1 = idx.shape[1]
    ix, ww = _neighbours(idx, w, sab)
    src = _cl_copy(feat, sab).transpose(0, 2, 1) if sab == "cl_swapped" else feat
    dt = np.float64 if f64 else np.float32
    acc = np.zeros((B, C, N1), dt)
    for k in range(3):
        g = np.take_along_axis(src, np.broadcast_to(ix[:, None, :, k], (B, C, N1)), axis=2).astype(dt)
        wk = np.broadcast_to(ww[:, None, :, k], (B, C, N1)).astype(dt)
        if fmad and not f64:
            acc = fma32(g, wk, acc)
        else:
            acc = acc + g * wk
    return _store_sabotage(acc, sab, IP_CG)


def scatter_np(contrib, ix, N, sab=None):
    """gin[b, c, j] = ((0 + v(t_0)) + v(t_1)) + ... over the positions t_0 < t_1 < ... with ix[b, t] == j, in the
    dtype of `contrib` (B, C, T); positions whose index is outside [0, N) count for nobody."""
    B, C, T = contrib.shape
    gin = np.zeros((B, C, N), contrib.dtype)
    for b in range(B):
        j = ix[b]
        ok = (j >= 0) & (j < N)
        if sab == "sentinel_first" and b == 0:
            for t in np.nonzero(~ok)[0]:
                gin[0, :, 0] += contrib[0, :, t]
        pos = np.nonzero(ok)[0]
        if sab == "descending":
            pos = pos[::-1]
        order = np.argsort(j[pos], kind="stable")
        sj, sp = j[pos][order], pos[order]
        n = len(sj)
        if n == 0:
            continue
        first = np.r_[True, sj[1:] != sj[:-1]]
        rank = np.arange(n) - np.maximum.accumulate(np.where(first, np.arange(n), 0))
        by_rank = np.argsort(rank, kind="stable")
        cuts = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2))
        for r in range(rank.max() + 1):
            m = by_rank[cuts[r]:cuts[r + 1]]
            gin[b][:, sj[m]] += contrib[b][:, sp[m]]
    return gin


def group_points_backward_np(gout, idx, N, sab=None, f64=False):
    B, C = gout.shape[:2]
    ix = idx.reshape(B, -1)
    if sab == "scene_base":
        ix = np.broadcast_to(ix[:1], ix.shape)
    elif sab == "idx_t1":
        ix = _shift(ix)
    return scatter_np(gout.reshape(B, C, -1).astype(np.float64 if f64 else np.float32), ix, N, sab)


def interp_contrib(gout, w, f64=False):
    """(B, C, 3 N1): gout[b, c, n] * w[b, n, k] at position 3 n + k, rounded to fp32 unless f64."""
    dt = np.float64 if f64 else np.float32
    B, C, N1 = gout.shape
    return (gout.astype(dt)[:, :, :, None] * w.astype(dt)[:, None, :, :]).reshape(B, C, 3 * N1)


def three_interpolate_backward_np(gout, idx, w, N2, sab=None, f64=False):
    ix, ww = _neighbours(idx, w, sab)
    return scatter_np(interp_contrib(gout, ww, f64), ix.reshape(idx.shape[0], -1), N2, sab)


def interp_add_np(y, sp, idx, w, bias, B, N1, N2, C, relu, sab=None, f64=False):
    """interp_add_cl_kernel in its documented order: a w0, + b w1, + c w2, then (y + acc) + bias, then ReLU; each
    operation rounded to fp32, or all of it in float64.  -> (B N1, C)."""
    dt = np.float64 if f64 else np.float32
    ix, ww = _neighbours(idx.astype(np.int64), w, sab)
    rows = sp.reshape(B, N2, C).astype(dt)
    if sab == "scene_base":
        rows = np.broadcast_to(rows[:1], rows.shape)
    acc = None
    for k in range(3):
        g = np.take_along_axis(rows, np.broadcast_to(ix[:, :, k, None], (B, N1, C)), axis=1)
        p = g * ww[:, :, k, None].astype(dt)
        acc = p if acc is None else acc + p
    yv = np.zeros((B, N1, C), dt) if y is None else y.reshape(B, N1, C).astype(dt)
    bb = bias.astype(dt)
    x = (acc + bb) + yv if sab == "bias_before_y" else (yv + acc) + bb
    if relu or sab == "relu_always":
        x = np.where(x > 0, x, dt(0))
    return x.reshape(B * N1, C)


def reference(c, inp, sab=None, f64=False):
    """The restatement of a case's operator on its inputs."""
    op = c["op"]
    if op in GROUP_OPS or op == "route_group":
        assert not f64
        return group_points_np(inp["feat"], inp["idx"], sab)
    if op in INTERP_OPS or op == "route_interp":
        return three_interpolate_np(inp["feat"], inp["idx"], inp["w"], c["fmad"], sab, f64)
    if op == "interp_add":
        return interp_add_np(inp["y"], inp["sp"], inp["idx"], inp["w"], inp["bias"], c["B"], c["N1"], c["N2"], c["C"],
                             c["relu"], sab, f64)
    if op == "group_bwd":
        return group_points_backward_np(inp["gout"], inp["idx"], c["N"], sab, f64)
    return three_interpolate_backward_np(inp["gout"], inp["idx"], inp["w"], c["N"], sab, f64)


def oracle_reference(O, c, inp):
    """The CPU oracle on a case (None where it has no such operator: interp_add_cl)."""
    op = c["op"]
    if op == "gather":
        return O.gather_points(inp["feat"], inp["idx"])
    if op in GROUP_OPS or op == "route_group":
        return O.group_points(inp["feat"], inp["idx"])
    if op in INTERP_OPS or op == "route_interp":
        return O.three_interpolate(inp["feat"], inp["idx"], inp["w"], fmad=c["fmad"])
    if op == "interp_add":
        return None
    twin = in_range_twin(c, inp)
    if op == "group_bwd":
        if bwd_T(c) == 0:
            return np.zeros((c["B"], c["C"], c["N"]), np.float32)
        return O.group_points_backward(twin["gout"], twin["idx"], c["N"])
    if bwd_T(c) == 0:
        return np.zeros((c["B"], c["C"], c["N"]), np.float32)
    return O.three_interpolate_backward(twin["gout"], twin["idx"], twin["w"], c["N"])


def atomic_bound(c, inp):
    """Per target: n_j 2^-23 sum |terms_j| (n_j contributions of an atomic backward in any order; 2^-23 is twice fp32's
    unit roundoff, which leaves room for the rounding of each product), and the float64 result."""
    op = c["op"]
    B = c["B"]
    if op == "group_bwd":
        terms = inp["gout"].reshape(B, c["C"], -1).astype(np.float64)
        ix = inp["idx"].reshape(B, -1)
    else:
        terms = interp_contrib(inp["gout"], inp["w"], f64=True)
        ix = inp["idx"].reshape(B, -1)
    want = scatter_np(terms, ix, c["N"])
    mag = scatter_np(np.abs(terms), ix, c["N"])
    count = scatter_np(np.ones_like(terms), ix, c["N"])
    return want, count * 2.0 ** -23 * mag
