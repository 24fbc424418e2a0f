"""CPU side of tests/f64_edges.py: the loop constants of csrc/ops_f64.hip are read out of the source as text and each
must be in the table of the axis it bounds with both neighbours; the float64 numpy models are the C oracle's double
build bit for bit on every forward case and on both backwards' exact family; every sabotaged model changes the result of
the case its table names; the constructions have the properties they are named for.  Every case runs: nothing is
sampled."""
import ctypes
import functools
import re

import numpy as np
import pytest

from tests import f64_edges as FE
from tests.test_dispatch_edges import CSRC, _one, _read


def read_constants():
    src = _read(CSRC, "ops_f64.hip")
    c = {}
    c["F64_FPS_THREADS"] = int(_one(r"^constexpr int F64_FPS_THREADS = (\d+);", src, "F64_FPS_THREADS"))
    _one(r"for \(int j = t; j < N; j \+= F64_FPS_THREADS\) \{", src, "the strided point loop")
    c["BQ_WAVES"] = int(_one(r"const int m = blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 6\);", src, "centroids per workgroup"))
    _one(r"const dim3 grid\(\(unsigned\)\(\(M \+ %d\) / %d\), \(unsigned\)B\);" % (c["BQ_WAVES"] - 1, c["BQ_WAVES"]), src,
         "ball query grid")
    c["BQ_STEP"] = int(_one(r"for \(int j0 = 0; j0 < N && cnt < K; j0 \+= (\d+)\) \{", src, "ball query step"))
    _one(r"for \(int s = cnt \+ lane; s < K; s \+= %d\) o\[s\] = cnt \? first : 0;" % c["BQ_STEP"], src, "padding stride")
    blocks = set(re.findall(r"blockIdx\.x \* (\d+) \+ threadIdx\.x;", src))
    assert len(blocks) == 1, blocks
    c["EW_THREADS"] = int(blocks.pop())
    assert len(re.findall(r"blockIdx\.x \* %d \+ threadIdx\.x;" % c["EW_THREADS"], src)) == 5          # 3-NN and the four
    assert len(re.findall(r"\+ %d\) / %d\)" % (c["EW_THREADS"] - 1, c["EW_THREADS"]), src)) == 5       # ... their grids
    assert len(re.findall(r"__launch_bounds__\(%d\)" % c["EW_THREADS"], src)) == 5 + 1                  # and the ball query
    lo_hi = _one(r"return cnt > (\d+) \? (\d+) : \(cnt < (\d+) \? (\d+) : cnt\);", src, "ref_block_lg_f64")
    assert lo_hi[0] == lo_hi[1] and lo_hi[2] == lo_hi[3]
    c["FPS_LG_MAX"], c["FPS_LG_MIN"] = int(lo_hi[0]), int(lo_hi[2])
    c["NN_SENTINEL"] = float(_one(r"double b0 = (1e\d+), b1 = 0\.0, b2 = 0\.0;", src, "3-NN sentinel"))
    return c


@pytest.fixture(scope="module")
def src():
    return read_constants()


@pytest.fixture(autouse=True)
def _double_oracle(oracle):
    with oracle.double_dispatch():
        yield


@functools.lru_cache(maxsize=None)
def _model(cid, sab=None, family="natural"):
    c = CASES[cid]
    op = c["op"]
    if op == "fps":
        return (FE.fps_np(FE.fps_inputs(c), c["M"], c["fmad"], sab),)
    if op == "bq":
        p, ctr, r = FE.bq_inputs(c)
        return FE.ball_query_np(p, ctr, r, c["K"], c["fmad"], sab)
    if op == "nn":
        q, k = FE.nn_inputs(c)
        return FE.three_nn_np(q, k, c["fmad"], sab)
    return (FE.ew_model(c, FE.ew_inputs(c, family), sab),)


CASES = {FE.case_id(c): c for c in FE.all_cases()}


def test_case_ids_are_unique():
    assert len(CASES) == len(FE.all_cases())


def test_constants_are_the_source(src):
    for name, value in src.items():
        assert getattr(FE, name) == value, name


def _neighbours(T, have, what):
    assert {T - 1, T, T + 1} <= set(have), (what, T, sorted(have))


def test_every_constant_is_in_its_table_with_both_neighbours(src):
    T = src["F64_FPS_THREADS"]
    for edge in (T, 2 * T, 1 << src["FPS_LG_MIN"], 1 << src["FPS_LG_MAX"], 64):        # strides, the clamp, one wave
        _neighbours(edge, FE.FPS_N, "FPS N")
    assert {1, 2, 3 * T + 1} <= set(FE.FPS_N)
    for edge in (src["BQ_STEP"], 2 * src["BQ_STEP"]):
        _neighbours(edge, FE.BQ_N, "ball query N")
        _neighbours(edge if edge == src["BQ_STEP"] else src["BQ_STEP"], FE.BQ_K, "ball query K")
    assert {1, 1000} <= set(FE.BQ_N) and {1, 2, 200} <= set(FE.BQ_K)
    _neighbours(src["BQ_WAVES"], FE.BQ_M, "ball query M")
    assert {m % src["BQ_WAVES"] for m in FE.BQ_M} == set(range(src["BQ_WAVES"])) and {1, 2, 301} <= set(FE.BQ_M)
    _neighbours(src["EW_THREADS"], FE.NN_N1, "3-NN N1")
    _neighbours(src["EW_THREADS"], FE.EW_S, "M K / N1")
    _neighbours(4, FE.NN_N2, "3-NN N2")                                                   # N2 >= 3: 3, 4, 5
    assert {1, 1001} <= set(FE.NN_N1) and {64, 1000} <= set(FE.NN_N2) and {1, 1000} <= set(FE.EW_S)


def test_every_axis_value_and_every_construction_is_used():
    fps, bq, nn, ew = FE.fps_cases(), FE.bq_cases(), FE.nn_cases(), FE.ew_cases()
    for N in FE.FPS_N:
        for kind in FE.FPS_KINDS:
            ms = {c["M"] for c in fps if c["N"] == N and c["kind"] == kind and not c["fmad"]}
            assert {N, 1} <= ms and (N <= 2 or any(1 < m < N for m in ms)), (N, kind)
    lg = lambda N: (N <= 16, N <= 512, N <= 1024)
    assert len({lg(c["N"]) for c in fps if c["fmad"]}) == 4
    assert {"coincident", "nonfinite"} <= {c["kind"] for c in fps}
    assert {c["N"] for c in bq} == set(FE.BQ_N) and {c["M"] for c in bq} == set(FE.BQ_M)
    assert {c["K"] for c in bq} == set(FE.BQ_K) and {c["kind"] for c in bq} == set(FE.BQ_KINDS) | {"nonfinite"}
    assert {c["N1"] for c in nn} == set(FE.NN_N1) and {c["N2"] for c in nn} == set(FE.NN_N2)
    assert {c["kind"] for c in nn} == set(FE.NN_KINDS) and any(c["fmad"] for c in nn)
    for op in FE.EW_OPS:
        mine = [c for c in ew if c["op"] == op]
        assert {c["S"] for c in mine} == set(FE.EW_S) and {c["C"] for c in mine} == set(FE.EW_C), op
        assert {c["N"] for c in mine} == set(FE.EW_N) and any(c["kind"] == "hot" for c in mine), op
        assert all(FE.mk_of(c)[1] == 1 for c in mine) == (op == "gather")
    assert {c["fmad"] for c in ew if c["op"] == "interp"} == {0, 1}


def test_fma64_is_the_c_library_fma():
    libm = ctypes.CDLL("libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    rng = np.random.default_rng(11)
    n = 4000
    a = rng.standard_normal(n) * np.exp(rng.uniform(-30, 45, n))
    b = rng.standard_normal(n) * np.exp(rng.uniform(-30, 45, n))
    c = np.where(rng.random(n) < 0.5, -a * b * (1.0 + rng.standard_normal(n) * 2.0 ** -30), rng.standard_normal(n))
    a[:4], b[:4], c[:4] = (np.nan, np.inf, 2.0, -0.0), (1.0, 0.0, np.inf, 3.0), (1.0, 1.0, -np.inf, 0.0)
    want = np.array([libm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert FE.same(FE.fma64(a, b, c), want)


# ------------------------------------------------------------------------------------------------------ model == oracle
@pytest.mark.parametrize("cid", [i for i, c in CASES.items() if c["op"] == "fps"])
def test_fps_model_is_the_oracle(oracle, cid):
    c = CASES[cid]
    pts = FE.fps_inputs(c)
    got = _model(cid)[0]
    assert np.array_equal(got, oracle.fps(pts, c["M"], fmad=c["fmad"]))
    if c["N"] <= 1025:
        assert np.array_equal(got, oracle.fps_literal(pts, c["M"], fmad=c["fmad"]))      # the 512-thread emulation
    if c["kind"] == "coincident":
        assert (got == 0).all()
    if c["kind"] == "nonfinite":                   # the infinite point is the farthest, and stays it (:85-90): NaN never
        assert (got[:, 1:] == 5).all()


@pytest.mark.parametrize("cid", [i for i, c in CASES.items() if c["op"] == "bq"])
def test_ball_query_model_is_the_oracle(oracle, cid):
    c = CASES[cid]
    pts, ctr, r = FE.bq_inputs(c)
    idx, cnt = _model(cid)
    oi, oc = oracle.ball_query(pts, ctr, r, c["K"], fmad=c["fmad"])
    assert np.array_equal(idx, oi) and np.array_equal(cnt, oc)
    # the constructed ball is what its kind says
    K, N = c["K"], c["N"]
    inside, sphere = FE.bq_hits(c)
    row, n = idx[:, c["M"] - 1], cnt[:, c["M"] - 1]
    if c["kind"] not in ("natural", "nonfinite", "empty"):
        want = inside[:K] + [inside[0]] * (K - len(inside[:K]))
        assert (row == np.array(want)).all() and (n == min(K, len(inside))).all()
    if c["kind"] == "empty":
        assert (cnt == 0).all() and (idx == 0).all()
    if c["kind"] == "last":
        assert inside == [N - 1]
    if c["kind"] == "lane63":
        assert len(inside) == K and inside[-1] % FE.BQ_STEP == FE.BQ_STEP - 1
    if c["kind"] == "straddle":
        s = inside[-1] // FE.BQ_STEP
        assert sum(j // FE.BQ_STEP < s for j in inside) == K - 1 and sum(j // FE.BQ_STEP == s for j in inside) == 3
    if c["kind"] == "late":
        assert len(inside) == K + 2 and inside[K] // FE.BQ_STEP > inside[K - 1] // FE.BQ_STEP
    if c["kind"] == "short_pad":
        assert (K - n > FE.BQ_STEP).all() and inside[0] > 0
    if c["kind"] == "exact_r":
        assert len(sphere) >= 3 and not set(sphere) & set(row.reshape(-1).tolist())
        d = pts[:, :, sphere] - ctr[:, :, c["M"] - 1:]
        assert ((d * d).sum(axis=1) == FE.RADIUS ** 2).all()                              # exactly r: excluded


@pytest.mark.parametrize("cid", [i for i, c in CASES.items() if c["op"] == "nn"])
def test_three_nn_model_is_the_oracle(oracle, cid):
    c = CASES[cid]
    q, k = FE.nn_inputs(c)
    idx, d2 = _model(cid)
    oi, od = oracle.three_nn(q, k, fmad=c["fmad"])
    assert np.array_equal(idx, np.where(oi < 0, 0, oi)) and FE.same(d2, od)             # the library's index rule
    w = FE.interp_weights_np(d2)
    assert np.allclose(w, oracle.interp_weights(d2), rtol=1e-15, atol=0)
    if c["kind"] == "coincident":
        assert (idx == np.arange(3)).all() and (d2 == 0).all()
    if c["kind"] == "sentinel":
        # beside two far keys, beside one, beside none; and the query that is 1e21 away from everything
        assert idx[0, 0].tolist() == [1, c["N2"] - 1, 0] and d2[0, 0].tolist() == [1.0, 4.0, 1e40]
        assert idx[1, 0].tolist() == [2, 0, 0] and d2[1, 0].tolist() == [1.0, 1e40, 0.0]
        assert idx[2, 0].tolist() == [0, 0, 0] and d2[2, 0].tolist() == [1e40, 0.0, 0.0]
        assert (idx[:, -1] == 0).all() and (d2[:, -1] == np.array([1e40, 0.0, 0.0])).all()
        assert (oi[0, 0, 2], oi[1, 0, 1], oi[2, 0, 0]) == (-1, -1, -1)                   # what the reference writes there
        assert (d2 <= 1e40).all()                                                        # 1e42 never enters
    if c["kind"] == "nonfinite":
        assert (idx[:, 2] == 0).all() and (idx[:, 4] == 0).all() and (d2[:, 2, 0] == 1e40).all()
        assert not np.isin(idx, (1, 3)).any() or c["N2"] > 5


@pytest.mark.parametrize("cid", [i for i, c in CASES.items() if c["op"] in FE.EW_OPS])
def test_data_movement_models_are_the_oracle(oracle, cid):
    c = CASES[cid]
    for family in ("exact", "natural"):
        if c["op"].endswith("_bwd") and family == "natural":
            continue                                # the order of a backward's sums is the oracle's own only there
        inp = FE.ew_inputs(c, family)
        assert FE.same(_model(cid, None, family)[0], FE.ew_oracle(oracle, c, inp)), family
    if c["kind"] == "signed_zero":
        out = _model(cid)[0]
        assert (out == 0).sum() > 3 * c["S"] and not np.signbit(out[out == 0]).any()     # acc starts from +0.0


def test_exact_family_is_exact_in_any_order():
    """Quarter-integers below 2^40: the sums of the exact family are the same double in the reverse order too."""
    for c in FE.ew_cases():
        if not c["op"].endswith("_bwd"):
            continue
        inp = FE.ew_inputs(c, "exact")
        want = FE.ew_model(c, inp)
        if c["op"] == "group_bwd":
            g = inp["gout"].reshape(FE.B, c["C"], -1)
            got = FE._scatter(g[:, :, ::-1], inp["idx"].reshape(FE.B, -1)[:, ::-1], c["N"], None)
        else:
            got = FE.three_interpolate_backward_np(inp["gout"][:, :, ::-1], inp["idx"][:, ::-1, ::-1],
                                                   inp["w"][:, ::-1, ::-1], c["N"])
        assert FE.same(got, want), FE.case_id(c)
        assert (np.abs(want) < 2.0 ** 40).all() and (want == np.round(want * 4) / 4).all()


# ------------------------------------------------------------------------------------------------------ sabotage
SEEN_BY = {
    # FPS
    ("fps", "f32_coords"): "fps-N=65-M=65-double_only",
    ("fps", "tie_lowest_index"): "fps-N=17-M=8-lattice",
    ("fps", "no_clamp"): "fps-N=1025-M=1025-lattice",
    ("fps", "skip_1024"): "fps-N=1025-M=512-uniform64",
    ("fps", "min_not_stored"): "fps-N=15-M=7-uniform64",
    ("fps", "no_d_guard"): "fps-N=63-M=63-lattice",
    # ball query
    ("bq", "le"): "bq-N=63-M=4-K=63-exact_r",
    ("bq", "pad_zero"): "bq-N=128-M=5-K=200-short_pad",
    ("bq", "tail_read"): "bq-N=1000-M=4-K=63-natural",
    ("bq", "f32_dist"): "bq-N=1000-M=3-K=64-exact_r",
    ("bq", "cnt_unclamped"): "bq-N=65-M=3-K=1-straddle",
    # 3-NN
    ("nn", "le"): "nn-N1=257-N2=1000-lattice",
    ("nn", "f32_dist"): "nn-N1=257-N2=64-double_only",
    ("nn", "inf_sentinel"): "nn-N1=255-N2=3-sentinel",
    ("nn", "minus1"): "nn-N1=257-N2=64-sentinel",
    # group / gather / interpolate / backwards
    ("group", "batch_offset"): "group-N=300-S=257-C=3-plain",
    ("group", "chan_extent"): "group-N=300-S=257-C=3-plain",
    ("group", "last_block"): "group-N=300-S=257-C=3-plain",
    ("gather", "batch_offset"): "gather-N=7-S=255-C=1-plain",
    ("gather", "chan_extent"): "gather-N=7-S=255-C=1-plain",
    ("gather", "last_block"): "gather-N=7-S=255-C=1-plain",
    ("interp", "batch_offset"): "interp-N=300-S=257-C=3-plain",
    ("interp", "chan_extent"): "interp-N=300-S=257-C=3-plain",
    ("interp", "last_block"): "interp-N=300-S=257-C=3-plain-fmad",
    ("interp", "weights_rotated"): "interp-N=7-S=1-C=1-plain",
    ("interp", "assoc_swapped"): "interp-N=300-S=256-C=3-plain",
    ("group_bwd", "batch_offset"): "group_bwd-N=300-S=257-C=3-plain",
    ("group_bwd", "chan_extent"): "group_bwd-N=300-S=257-C=3-plain",
    ("group_bwd", "last_block"): "group_bwd-N=1-S=257-C=3-hot",
    ("interp_bwd", "batch_offset"): "interp_bwd-N=300-S=257-C=3-plain",
    ("interp_bwd", "chan_extent"): "interp_bwd-N=300-S=257-C=3-plain",
    ("interp_bwd", "last_block"): "interp_bwd-N=300-S=257-C=3-hot",
    ("interp_bwd", "weights_rotated"): "interp_bwd-N=7-S=1-C=1-plain",
}


def _sabotages_of(op):
    if op in FE.EW_OPS:
        return [s for s in FE.EW_SABOTAGES if (op, s) in SEEN_BY]
    return list({"fps": FE.FPS_SABOTAGES, "bq": FE.BQ_SABOTAGES, "nn": FE.NN_SABOTAGES}[op])


def test_every_listed_sabotage_has_a_case():
    for op, table in (("fps", FE.FPS_SABOTAGES), ("bq", FE.BQ_SABOTAGES), ("nn", FE.NN_SABOTAGES)):
        assert {s for o, s in SEEN_BY if o == op} == set(table)
    for op in FE.EW_OPS:
        want = {"batch_offset", "chan_extent", "last_block"}
        if op.startswith("interp"):
            want.add("weights_rotated")
        if op == "interp":
            want.add("assoc_swapped")              # the backward's product has one association
        assert {s for o, s in SEEN_BY if o == op} == want, op
    assert all(cid in CASES and CASES[cid]["op"] == op for (op, _), cid in SEEN_BY.items())


@pytest.mark.parametrize("op,sab", sorted(SEEN_BY))
def test_sabotaged_model_is_seen(op, sab):
    """Each wrong-kernel variant of a model changes the result of the case named for it:

    operator    sabotage           seen by                               because
    fps         f32_coords         N=65 M=65 double_only                 the pair member 2^-40 farther out ties again in fp32
    fps         tie_lowest_index   N=17 M=8 lattice                      index 2 beats index 1 under the reversed key
    fps         no_clamp           N=1025 M=1025 lattice                 11 reversed bits order j and j + 512 differently
                                   (the lower clamp cannot show: reversing j < 16 over fewer bits keeps the order)
    fps         skip_1024          N=1025 M=512 uniform64                point 1024 is never picked
    fps         min_not_stored     N=15 M=7 uniform64                    distances to the current point only
    fps         no_d_guard         N=63 M=63 lattice                     M = N with coincident points: index 0 instead of a repeat
    ball query  le                 N=63 M=4 K=63 exact_r                 the points at exactly r enter
    ball query  pad_zero           N=128 M=5 K=200 short_pad             198 padding slots, first hit 64
    ball query  tail_read          N=1000 M=4 K=63 natural               lanes 1000 .. 1023 of the last step read y, z and the next scene
    ball query  f32_dist           N=1000 M=3 K=64 exact_r               r^2 (1 - 2^-39) rounds to r^2
    ball query  cnt_unclamped      N=65 M=3 K=1 straddle                 three hits in the step, one slot
    3-NN        le                 N1=257 N2=1000 lattice                the later of two equidistant keys moves in front
    3-NN        f32_dist           N1=257 N2=64 double_only              the later, nearer key ties with the earlier one
    3-NN        inf_sentinel       N1=255 N2=3 sentinel                  a key 1e21 away enters
    3-NN        minus1             N1=257 N2=64 sentinel                 slot 2 / slot 1 / slot 0 keep -1
    group ...   batch_offset       S=257 C=3 N=300 (gather: S=255 C=1)   scene 0's indices for every scene
    group ...   chan_extent        the same                              row (b, c) taken from (b C + c) S
    group ...   last_block         the same; the hot cases of the backwards   element 256 of 257 (of 255: all) missing
    interp ...  weights_rotated    S=1 C=1 N=7                           w2, w0, w1
    interp      assoc_swapped      S=256 C=3 N=300                       fma chain against rounded products
    """
    cid = SEEN_BY[(op, sab)]
    honest, wrong = _model(cid), _model(cid, sab)
    assert not all(FE.same(a, b) for a, b in zip(honest, wrong)), (cid, sab)


# ------------------------------------------------------------------------------------------------------ constructions
@pytest.mark.parametrize("N", FE.FPS_N)
def test_fps_constructions(N):
    """uniform64 holds no float; the lattice has fewer positions than points and, by construction, a tie between two
    waves (N > 69) and between two strides of one thread (N > 1031); the double-only pairs tie in fp32 alone."""
    M = N
    for kind in FE.FPS_KINDS:
        c = dict(op="fps", N=N, M=M, kind=kind, fmad=0)
        pts = FE.fps_inputs(c)
        assert pts.dtype == np.float64 and pts.shape == (FE.B, 3, N)
        as32 = pts.astype(np.float32).astype(np.float64)
        if kind == "uniform64":
            assert (as32 != pts).all()
            continue
        if N >= 64:
            assert all(len(np.unique(pts[b].T, axis=0)) < N for b in range(FE.B))
        pairs = FE.fps_pairs(N)
        assert ((5, 69) in pairs) == (N > 69) and ((7, 7 + FE.F64_FPS_THREADS) in pairs) == (N > 7 + FE.F64_FPS_THREADS)
        for a, b in pairs:
            assert (as32[:, :, a] == as32[:, :, b]).all()
            assert (pts[:, :, a] == pts[:, :, b]).all() == (kind == "lattice")
        got = _model(FE.case_id(c))[0]
        if kind == "lattice":
            for b in range(FE.B):                                              # the corner pairs tie in the first picks
                ties = {}
                FE.fps_np(pts[b:b + 1], min(M, 5), 0, None, ties)
                assert ties.get("count", 0) > 0 or N < 15
                assert ties.get("waves", False) or N <= 69, (N, b)
                assert ties.get("strides", False) or N <= 7 + FE.F64_FPS_THREADS, (N, b)
            # M = N on a cloud with coincident points: the picks end in a repeated index
            if N >= 64:
                assert (got[:, -1] == got[:, -2]).all()
        elif pairs:
            assert not np.array_equal(got, FE.fps_np(as32, M))              # the ties come back in fp32, the picks differ
            moved = [b if FE.fps_tie_key(N, a) < FE.fps_tie_key(N, b) else a for a, b in pairs]
            assert all((got[:, :len(pairs) + 1] == m).any(axis=1).all() for m in moved)   # double picks the farther one


def test_three_nn_double_only_pairs_tie_in_fp32():
    c = CASES["nn-N1=257-N2=64-double_only"]
    q, k = FE.nn_inputs(c)
    d = FE.dist2_64(k[:, 0, None, :], k[:, 1, None, :], k[:, 2, None, :], q[:, 0, :, None], q[:, 1, :, None], q[:, 2, :, None])
    early, late = d[:, :, 0::2], d[:, :, 1::2]
    nearer = late < early
    assert nearer.mean() > 0.2                                                          # every query right of the pair
    assert (late.astype(np.float32)[nearer] == early.astype(np.float32)[nearer]).all()
    idx = _model(FE.case_id(c))[0]
    assert (idx[:, :, 0] % 2 == 1).mean() > 0.2                                         # ... and the later key leads


def test_natural_family_spans_the_magnitudes():
    c = CASES["interp_bwd-N=300-S=1000-C=3-plain"]
    g = np.abs(FE.ew_inputs(c, "natural")["gout"])
    assert g.max() / np.median(g) > 100 and np.median(g) / g[g > 0].min() > 100
    assert (g.astype(np.float32).astype(np.float64) != g).mean() > 0.99
    for op in ("group_bwd", "interp_bwd"):
        hot = FE.ew_inputs(CASES["%s-N=300-S=257-C=3-hot" % op], "natural")["idx"]
        assert all(len(np.unique(hot[b])) == 1 for b in range(FE.B))
        plain = FE.ew_inputs(CASES["%s-N=300-S=257-C=3-plain" % op], "natural")["idx"]
        assert all({0, 299} <= set(plain[b].reshape(-1).tolist()) for b in range(FE.B))
