"""CPU side of the dispatch ladder (tests/dispatch_edges.py): the thresholds are read out of the sources as text and
every one of them must be in the ladder with its neighbours, every kernel form at both ends of its range, every stated
form the one the dispatcher's own constants give.  A boundary that moves, or a new kernel case, fails here until the
ladder follows.  The inputs are checked too: the lattice clouds do tie, the tie-free clouds are tie-free, and the
yardsticks (the oracle at the smallest sizes, the numpy restatement of the distance contract) agree with each other
before a GPU is involved."""
import ctypes
import ctypes.util
import os
import re

import numpy as np
import pytest

from tests import dispatch_edges as DE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "s4g_release_amd", "csrc")


def _read(*parts):
    return open(os.path.join(*parts)).read()


def _one(pattern, text, what):
    """The single match of an anchored pattern; a name that disappeared (or doubled) fails, it never passes empty."""
    found = re.findall(pattern, text, flags=re.M)
    assert len(found) == 1, "%s: expected exactly one match of %r, found %d" % (what, pattern, len(found))
    return found[0]


def _prod(groups):
    out = 1
    for g in groups:
        out *= int(g)
    return out


def _body(text, signature):
    """Text of the function whose head contains `signature`, up to the first closing brace in column 0."""
    start = text.index(signature)
    return text[start:text.index("\n}", start)]


def read_thresholds(csrc=CSRC, functions_py=os.path.join(ROOT, "s4g_release_amd", "functions.py")):
    """Every threshold the three dispatchers compare against, by the name it has in the source."""
    fps = _read(csrc, "fps.hip")
    bq = _read(csrc, "ball_query.hip")
    nn = _read(csrc, "three_nn.hip")
    grid = _read(csrc, "grid.h")
    fn = _read(functions_py)
    c = {}
    c["reg"] = [(int(t), int(p)) for t, p in re.findall(r"^\s*S4G_FPS_CASE\((\d+),\s*(\d+)\)", fps, flags=re.M)]
    c["pruned"] = [(int(t), int(p)) for t, p in re.findall(r"^\s*S4G_FPS_PRUNED\((\d+),\s*(\d+)\)", fps, flags=re.M)]
    c["l2_cap"] = _prod(_one(r"^constexpr int FPS_L2_CAP = (\d+) \* (\d+);", fps, "FPS_L2_CAP"))
    c["l2_cap_big"] = int(_one(r"^constexpr int FPS_L2_CAP_BIG = (\d+);", fps, "FPS_L2_CAP_BIG"))
    c["min_picks"] = int(_one(r"^constexpr int FPS_PRUNED_MIN_PICKS = (\d+);", fps, "FPS_PRUNED_MIN_PICKS"))
    _one(r"M > FPS_PRUNED_MIN_PICKS\b", fps, "launch_fps' use of FPS_PRUNED_MIN_PICKS")
    up = _body(fps, "static bool fps_use_pruned(")
    c["pruned_top"] = _prod(_one(r"if \(N > \(int64_t\)(\d+) \* (\d+)\) return false;", up, "fps_use_pruned top"))
    c["forced_pruned_above"] = _prod(_one(r"e\[0\] == 'p'\) return N > (\d+) \* (\d+);", up, "fps_use_pruned forced"))
    d = _one(r"return N > (\d+) \* (\d+) \|\| \(N > (\d+) \* (\d+) && \(M < 0 \|\| M >= (\d+)\)\);", up,
             "fps_use_pruned default")
    c["pruned_above"], c["long_chain_above"], c["long_chain_picks"] = _prod(d[0:2]), _prod(d[2:4]), int(d[4])
    ul = _body(fps, "static bool fps_use_pruned_l2(")
    d = _one(r"if \(N <= \(int64_t\)(\d+) \* (\d+) \|\| N > FPS_L2_CAP_BIG \|\| M < (\d+)\) return false;", ul,
             "fps_use_pruned_l2")
    c["l2_above"], c["l2_min_picks"] = _prod(d[0:2]), int(d[2])
    c["l2_slots"] = [int(s) for s in _one(r"return N <= FPS_L2_CAP \? (\d+) : (\d+);", fps, "fps_l2_slots")]
    c["gr_max_points"] = int(_one(r"^constexpr int GR_MAX_POINTS = (\d+);", grid, "GR_MAX_POINTS"))
    ug = _body(bq, "static bool bq_use_grid(")
    c["bq_max_k"] = int(_one(r"if \(N > GR_MAX_POINTS \|\| K > (\d+)\) return false;", ug, "bq_use_grid K"))
    c["bq_min_n"] = int(_one(r"return N >= (\d+);", ug, "bq_use_grid N"))
    us = _body(nn, "static int launch_three_nn_scan(")
    c["nn_split"] = [int(v) for v in _one(r"N2 >= (\d+) && N2 <= (\d+);", us, "three_nn split range")]
    c["nn_split_wide"] = int(_one(r"if \(N2 >= (\d+)\) \{", us, "three_nn split width"))
    c["nn_split_lanes"] = sorted(int(v) for v in re.findall(r"three_nn_split_kernel<FMAD, WEIGHTS, IdxT, (\d+)>", us))
    _one(r"N2 > GR_MAX_POINTS \|\|", _body(nn, "static int launch_three_nn_grid("), "three_nn grid limit")
    c["nn_grid"] = [int(v) for v in _one(r"use_grid = \((\d+) <= N2 <= (\d+) and", fn, "functions.py 3-NN routing")]
    return c


@pytest.fixture(scope="module")
def src():
    return read_thresholds()


def test_the_sources_still_carry_every_name(src):
    assert len(src["reg"]) >= 8 and len(src["pruned"]) >= 4
    assert src["reg"] == sorted(src["reg"], key=lambda tp: tp[0] * tp[1])          # first match = smallest that fits
    assert src["pruned"] == sorted(src["pruned"], key=lambda tp: tp[0] * tp[1])
    top = max(t * p for t, p in src["reg"])
    assert src["pruned_top"] == top == src["l2_above"] == max(t * p for t, p in src["pruned"])
    assert src["l2_slots"] == [100, 128] and src["l2_cap"] == 512 * 100
    assert src["nn_grid"][1] == src["gr_max_points"]
    assert src["nn_split_lanes"] == [4, 8]


def test_ladders_are_not_empty_and_have_no_duplicates():
    for cases in (DE.fps_cases(), DE.bq_cases(), DE.nn_cases(), DE.FPS_FMAD, DE.FPS_PICK_DISTANCES, DE.FPS_WORKSPACE,
                  DE.NN_GRID_ENTRY_N2):
        assert len(cases) > 0
        assert len(set(cases)) == len(cases)
    keys = [(N, M, mode) for N, M, mode, _ in DE.fps_cases()]
    assert len(set(keys)) == len(keys)
    assert {mode for _, _, mode, _ in DE.fps_cases()} == {"default", "pruned", "dense"}
    for N, M, _, _ in DE.fps_cases():
        assert 0 < M <= N and N * M <= 3e8                                        # the oracle's O(N M) stays affordable


def test_every_fps_case_states_the_form_the_dispatcher_gives(src):
    for N, M, mode, form in DE.fps_cases():
        assert DE.fps_form(N, M, mode, src) == form, (N, M, mode)
    by_key = {(N, M, mode): form for N, M, mode, form in DE.fps_cases()}
    for N, M, mode in DE.FPS_FMAD + DE.FPS_PICK_DISTANCES:
        assert (N, M, mode) in by_key, (N, M, mode)                               # a ladder entry: its form is stated
    forms = {by_key[k].split("<")[0] for k in DE.FPS_PICK_DISTANCES}
    assert forms == {"reg", "pruned", "l2"}                                       # the three forms that report D_k
    assert {by_key[k] for k in DE.FPS_FMAD} == set(by_key.values())                # one size per kernel form
    for N, M, mode, full, null, short in DE.FPS_WORKSPACE:
        assert DE.fps_form(N, M, mode, src) == full
        for other in (null, short):
            assert other == "EWORKSPACE" or other.split("<")[0] in ("reg", "stream")
    assert DE.FPS_MAY_PRUNE_ABOVE == {"default": src["long_chain_above"], "pruned": src["forced_pruned_above"]}
    assert DE.FPS_REG_TOP == src["pruned_top"] and DE.FPS_L2_TOP == src["l2_cap_big"]


def test_every_fps_threshold_is_in_the_ladder_with_its_neighbours(src):
    rows = {}
    for N, M, mode, form in DE.fps_cases():
        rows.setdefault((N, mode), {})[M] = form
    default_n = {N for N, mode in rows if mode == "default"}
    thresholds = {t * p for t, p in src["reg"]} | {src["l2_cap"], src["l2_cap_big"], src["pruned_above"],
                                                   src["long_chain_above"], src["forced_pruned_above"]}
    for T in sorted(thresholds):
        assert {T - 1, T, T + 1} <= default_n, T
    assert src["gr_max_points"] in default_n                                      # "the 16-bit positions end there" + 1
    # every kernel form at both ends of its range
    at = {}
    for N, M, mode, form in DE.fps_cases():
        at.setdefault(form, set()).add(N)
    lo = 1
    for t, p in src["reg"]:
        name = "reg<%d,%d>" % (t, p)
        assert name in at, name
        assert t * p in at[name] and (lo == 1 or lo in at[name]), name
        lo = t * p + 1
    lo = src["forced_pruned_above"] + 1
    for t, p in src["pruned"]:
        name = "pruned<%d,%d>" % (t, p)
        assert name in at, name
        assert t * p in at[name] and lo in at[name], name
        lo = t * p + 1
    assert {src["l2_above"] + 1, src["l2_cap"]} <= at["l2<512,100>"]
    assert {src["l2_cap"] + 1, src["l2_cap_big"]} <= at["l2<512,128>"]
    assert {src["l2_above"] + 1, src["l2_cap_big"], src["l2_cap_big"] + 1, src["l2_cap_big"] + 2} <= at["stream"]
    # the M thresholds, each on a row where it decides
    mp = src["min_picks"]
    for t, p in src["pruned"]:
        assert any(ms.get(mp, "").startswith("reg") and ms.get(mp + 1) == "pruned<%d,%d>" % (t, p)
                   for ms in rows.values()), (t, p)
    lm = src["l2_min_picks"]
    for slots in src["l2_slots"]:
        assert any(ms.get(lm - 1) == "stream" and ms.get(lm) == "l2<512,%d>" % slots for ms in rows.values()), slots
    lc = src["long_chain_picks"]
    decided = [N for (N, mode), ms in rows.items() if mode == "default" and
               ms.get(lc - 1, "").startswith("reg") and ms.get(lc, "").startswith("pruned")]
    assert src["long_chain_above"] + 1 in decided and src["pruned_above"] in decided
    assert rows[(src["long_chain_above"], "default")][lc].startswith("reg")       # N > 5 120 is strict
    # M = N at the small sizes
    small = [N for N, M, _, _ in DE.fps_cases() if M == N]
    assert len(small) >= 10 and min(small) < 256 and max(small) > 2560
    # the dense forms of the sizes the default mode prunes
    for t, p in src["reg"]:
        if t * p > src["pruned_above"]:
            assert rows[(t * p, "dense")], (t, p)


def test_ball_query_and_three_nn_thresholds_are_in_their_ladders(src):
    assert (DE.BQ_GRID_MIN_N, DE.BQ_GRID_MAX_N, DE.BQ_GRID_MAX_K) == (src["bq_min_n"], src["gr_max_points"],
                                                                      src["bq_max_k"])
    for T in (src["bq_min_n"] - 1, src["gr_max_points"]):
        assert {T, T + 1} <= set(DE.BQ_N), T
    assert {src["bq_max_k"], src["bq_max_k"] + 1, 1, 64} <= set(DE.BQ_K)
    assert DE.BQ_M % 4 != 0
    paths = {(N, K, mode): path for N, K, mode, path in DE.bq_cases()}
    assert paths[(src["bq_min_n"] - 1, 64, "auto")] == "scan" and paths[(src["bq_min_n"], 64, "auto")] == "grid"
    assert paths[(src["gr_max_points"], 64, "auto")] == "grid" and paths[(src["gr_max_points"] + 1, 64, "auto")] == "scan"
    assert paths[(src["bq_min_n"], src["bq_max_k"] + 1, "auto")] == "scan"
    assert (src["gr_max_points"] + 1, 64, "grid") not in paths and (src["bq_min_n"] - 1, 64, "grid") in paths

    assert (DE.NN_SPLIT_MIN, DE.NN_SPLIT_MAX) == tuple(src["nn_split"]) and DE.NN_SPLIT_WIDE == src["nn_split_wide"]
    assert (DE.NN_GRID_MIN, DE.NN_GRID_MAX) == tuple(src["nn_grid"])
    n2 = set(DE.NN_N2)
    for T in (3, src["nn_split"][0], src["nn_split_wide"], src["nn_split"][1], src["gr_max_points"]):
        assert {T, T + 1} <= n2 and (T == 3 or T - 1 in n2), T
    narrow, wide = src["nn_split_lanes"]
    assert any(src["nn_split"][0] <= n < src["nn_split_wide"] and n % narrow == 1 for n in n2)
    assert any(src["nn_split_wide"] <= n <= src["nn_split"][1] and n % wide == 1 for n in n2)
    assert DE.NN_N1 % 256 != 0
    assert {3, 4, src["gr_max_points"] - 1, src["gr_max_points"]} <= set(DE.NN_GRID_ENTRY_N2)
    assert max(DE.NN_GRID_ENTRY_N2) <= src["gr_max_points"] < max(DE.NN_N2)


def test_lattice_inputs_tie_and_kinds_follow_the_size():
    seen = set()
    for N, M, _, _ in DE.fps_cases():
        if (N, M) in seen:
            continue
        seen.add((N, M))
        clouds = DE.fps_inputs(N, M)
        assert ("tabletop" in clouds) == (N > 10240) and {"uniform", "lattice"} <= set(clouds)
        for kind, pts in clouds.items():
            assert pts.shape == (2, 3, N) and pts.dtype == np.float32 and np.isfinite(pts).all()
            assert not np.array_equal(pts[0], pts[1])                              # two DIFFERENT scenes
        assert DE.lattice_levels(N) ** 3 < N
        for b in range(2):
            assert DE.distinct_points(clouds["lattice"][b]) < N, (N, M, b)
    for N2 in DE.NN_N2:
        q, k = DE.nn_inputs(N2)["lattice"]
        assert q.shape == (2, 3, DE.NN_N1) and k.shape == (2, 3, N2)
        assert N2 < 100 or DE.distinct_points(k[0]) < N2


def test_oracle_agrees_with_its_literal_form_at_the_smallest_sizes(oracle):
    sizes = sorted({(N, M) for N, M, _, _ in DE.fps_cases()})[:8]
    for N, M in sizes:
        for kind, pts in DE.fps_inputs(N, M).items():
            for fmad in (0, 1):
                assert np.array_equal(oracle.fps(pts, M, fmad=fmad), oracle.fps_literal(pts, M, fmad=fmad)), (N, M, kind)


def test_fma32_is_the_fused_multiply_add():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(7)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 3, size=4000)).astype(np.float32)
    # a b = 1 + 2^-11 + 2^-24 exactly: halfway between two float32, so a sum rounded to double first forgets on which
    # side a tiny c puts it
    a[:4] = b[:4] = np.float32(1 + 2.0 ** -12)
    c[:4] = np.float32([2.0 ** -60, -2.0 ** -60, 2.0 ** -80, 0.0])
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert want[0] != want[1]
    assert np.array_equal(DE.fma32(a, b, c).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("fmad", [False, True])
def test_numpy_distance_contract_reproduces_the_oracles_picks(oracle, fmad):
    """The restatement that recomputes the pick distances on the GPU side is the oracle's arithmetic: in a numpy FPS
    over it the oracle's pick is the ONLY point that holds the maximum at every step, and D_k is that maximum."""
    N, M = 257, 257
    pts = DE.fps_inputs(N, M)["uniform"]
    idx = oracle.fps(pts, M, fmad=int(fmad))
    for b in range(2):
        D = DE.pick_distances(pts[b], idx[b], fmad)
        md = np.full(N, np.inf, np.float32)
        for k in range(1, M):
            md = np.minimum(md, DE.dist2(pts[b][:, idx[b, k - 1]:idx[b, k - 1] + 1], pts[b], fmad))
            assert md[idx[b, k]] == md.max() == D[k], (b, k)
            assert (md == md.max()).sum() == 1, (b, k)


@pytest.mark.parametrize("N,M,mode", DE.FPS_PICK_DISTANCES)
def test_pick_distance_inputs_are_tie_free_and_tied_as_labelled(oracle, N, M, mode):
    """What the GPU test expects of s4g_fps_prefix_check_f32, settled here: over the oracle's picks the tie-free cloud
    is a proven prefix and the lattice cloud is not, under both contracts."""
    clouds = DE.fps_inputs(N, M)
    M2 = DE.prefix_steps(M)
    for fmad in (False, True):
        for kind, proven in (("uniform", True), ("lattice", False)):
            pts = clouds[kind]
            idx = oracle.fps(pts, M, fmad=int(fmad))
            for b in range(2):
                D = DE.pick_distances(pts[b], idx[b], fmad)
                assert DE.prefix_is_proven(pts[b][:, idx[b]], D, M2, fmad) == proven, (kind, fmad, b)


def test_ball_query_radius_gives_empty_short_and_full_balls(oracle):
    for N in (min(DE.BQ_N), max(DE.BQ_N)):
        for K in DE.BQ_K:
            pts, ctr, r = DE.bq_inputs(N, K)
            _, cnt = oracle.ball_query(pts, ctr, r, K)
            assert DE.bq_has_all_ball_kinds(cnt, K), (N, K, r)
