"""CPU side of tests/gather_edges.py: the kernel constants and the routing literals are read out of the sources as text
and each must be in the case table of the axis it bounds with both neighbours; the numpy restatements are the oracle bit
for bit on every case; every sabotaged restatement changes the output of at least one case (the test prints which); the
exact input family really is exact.  Every case runs: nothing is sampled."""
import re

import numpy as np
import pytest

from tests import gather_edges as GE
from tests.test_dispatch_edges import CSRC, ROOT, _one, _read


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def read_constants():
    grp = _read(CSRC, "group.hip")
    itp = _read(CSRC, "interpolate.hip")
    sct = _read(CSRC, "scatter.hip")
    srt = _read(CSRC, "radix_sort.hip")
    fn = _read(ROOT, "s4g_release_amd", "functions.py")
    c = {}
    c["GP_THREADS"] = int(_one(r"^constexpr int GP_THREADS = (\d+);", grp, "GP_THREADS"))
    c["GP_CG"] = int(_one(r"^constexpr int GP_CG = (\d+);", grp, "GP_CG"))
    c["IP_THREADS"] = int(_one(r"^constexpr int IP_THREADS = (\d+);", itp, "IP_THREADS"))
    c["IP_CG"] = int(_one(r"^constexpr int IP_CG = (\d+);", itp, "IP_CG"))
    c["IPQ"] = int(_one(r"^constexpr int IPQ = (\d+);", itp, "IPQ"))
    c["IPT_CH"] = int(_one(r"^#define S4G_IPT_CH (\d+)", itp, "S4G_IPT_CH"))
    c["IPT_PTS"] = int(_one(r"^#define S4G_IPT_PTS (\d+)", itp, "S4G_IPT_PTS"))
    t = _one(r"__shared__ float tile\[(\d+)\]\[(\d+)\];", itp, "feat_to_channels_last tile")
    c["CL_TILE"] = int(t[0])
    assert int(t[1]) == c["CL_TILE"] + 1
    _one(r"c0 = blockIdx\.y \* %d, n0 = blockIdx\.x \* %d;" % (c["CL_TILE"], c["CL_TILE"]), itp, "channels-last tile origin")
    c["IA_ROWS"] = int(_one(r"^constexpr int IA_ROWS = (\d+);", itp, "IA_ROWS"))
    c["IA_THREADS"] = int(_one(r"const int rpb = (\d+) / lpr;", itp, "interp_add rows per pass"))
    _one(r"const int rpb = %d / \(int\)\(C / 4\);" % c["IA_THREADS"], itp, "interp_add host rows per pass")
    c["IA_MAX_C"] = int(_one(r"\(C & 3\) \|\| C > (\d+) \|\|", itp, "interp_add C limit"))
    xcd = re.findall(r"\(nslices \+ (\d+)\) / (\d+) \* (\d+)\)", itp)
    assert len(xcd) == 2 and len({v for m in xcd for v in (int(m[0]) + 1, int(m[1]), int(m[2]))}) == 1, xcd
    c["XCDS"] = int(xcd[0][1])
    assert len(re.findall(r"const int xcd = blockIdx\.x & %d, kk = blockIdx\.x >> 3;" % (c["XCDS"] - 1), itp)) == 2
    assert len(re.findall(r"if \(slice >= nslices\) return;", itp)) == 2
    c["SC_THREADS"] = int(_one(r"^constexpr int SC_THREADS = (\d+);", sct, "SC_THREADS"))
    c["SC_TILE"] = int(_one(r"^constexpr int SC_TILE = (\d+);", sct, "SC_TILE"))
    c["SC_CL_MIN_C"] = int(_one(r"^constexpr int SC_CL_MIN_C = (\d+);", sct, "SC_CL_MIN_C"))
    _one(r"const bool cl = C >= SC_CL_MIN_C && ws_bytes >= w\.total_cl;", sct, "scatter_det's choice of form")
    th = int(_one(r"^constexpr int RS_THREADS = (\d+), RS_WAVES = RS_THREADS / 64;", srt, "RS_THREADS"))
    ch = int(_one(r"^constexpr int RS_CHUNKS = (\d+);", srt, "RS_CHUNKS"))
    _one(r"^constexpr int RS_WAVE_ELEMS = 64 \* RS_CHUNKS;", srt, "RS_WAVE_ELEMS")
    _one(r"^constexpr int RS_TILE = RS_WAVE_ELEMS \* RS_WAVES;", srt, "RS_TILE")
    c["RS_TILE"] = 64 * ch * (th // 64)
    g = _one(r"if C == 3 and B > 0 and \(M \* K\) % 4 == 0 and M \* K >= (\d+):", fn, "xyz routing")
    h = _one(r"elif C % 4 == 0 and C >= (\d+) and B > 0 and M \* K >= (\d+):", fn, "channels-last grouping routing")
    i = _one(r"if C % 4 == 0 and C >= (\d+) and B \* N1 > 0 and N1 >= N2:", fn, "channels-last interpolation routing")
    assert int(g) == int(h[1]) and int(h[0]) == int(i)
    c["ROUTE_MIN_MK"], c["ROUTE_MIN_C"] = int(g), int(i)
    return c


@pytest.fixture(scope="module")
def src():
    return read_constants()


@pytest.fixture(scope="module")
def cases():
    return GE.all_cases()


def test_constants_are_the_sources(src):
    for name, value in src.items():
        assert getattr(GE, name) == value, name


def _neighbours(T, have, what):
    assert {T - 1, T, T + 1} <= set(have), (what, T, sorted(have))


def test_every_constant_is_in_its_table_with_both_neighbours(src, cases):
    def axis(pred, key):
        return {key(c) for c in cases if pred(c)}
    mk = lambda c: c["M"] * c["K"]
    is_form = lambda op, f: (lambda c: c["op"] == op and GE.form(c) == f)
    # group_points, vec4 form: GP_THREADS lanes of four slots, GP_CG channels per block row
    quads = {v // 4 for v in axis(is_form("group", "vec4"), mk)}
    _neighbours(src["GP_THREADS"], quads, "vec4 lanes")
    assert 1 in quads
    _neighbours(src["GP_CG"], axis(is_form("group", "vec4"), lambda c: c["C"]), "vec4 channel group")
    assert {1, 2 * src["GP_CG"] + 1} <= axis(is_form("group", "vec4"), lambda c: c["C"])
    assert {1, 3} <= axis(is_form("group", "vec4"), lambda c: c["B"])
    # scalar form
    sc = axis(is_form("group", "scalar"), mk)
    _neighbours(src["GP_THREADS"], sc, "scalar lanes")
    assert {1, 3, 5, 4 * src["GP_THREADS"] - 1, 4 * src["GP_THREADS"]} <= sc
    assert any(c["mis"].get("idx") == 8 for c in cases if c["op"] == "group")
    assert any(c["mis"].get("out") == 4 for c in cases if c["op"] == "group")
    _neighbours(src["GP_THREADS"], axis(lambda c: c["op"] == "gather", lambda c: c["M"]), "gather_points")
    # xyz form
    aos = [c for c in cases if c["op"] == "group_xyz" and GE.form(c) == "aos"]
    _neighbours(src["GP_THREADS"], {mk(c) // 4 for c in aos}, "xyz lanes")
    _neighbours(src["GP_THREADS"], {c["N"] for c in aos}, "xyz_to_aos lanes")
    assert 1 in {c["N"] for c in aos} and 4 in {mk(c) for c in aos}
    fb = [c for c in cases if c["op"] == "group_xyz" and GE.form(c) != "aos"]
    assert {c["ws"] for c in fb} >= {"null", "short", "misaligned"}
    assert {k for c in fb for k in c["mis"]} == {"idx", "out"} and any(mk(c) % 4 for c in fb)
    # the two 64 x 64 tile kernels and the 32 x 32 channels-last copy in front of them
    for op, s_of, n_of in (("group_ws", mk, lambda c: c["N"]), ("interp_ws", lambda c: c["N1"], lambda c: c["N2"])):
        for fmad in ((0, 1) if op == "interp_ws" else (0,)):
            tile = [c for c in cases if c["op"] == op and GE.form(c) == "tile" and c.get("fmad", 0) == fmad]
            S = {s_of(c) for c in tile}
            for T in (src["IPT_PTS"], 2 * src["IPT_PTS"]):
                _neighbours(T, S, op + " points")
            assert {1, 3, 4, src["IPT_PTS"] + 2} <= S                                     # S % 4 of 0, 1, 2, 3 at the tile edge
            C = {c["C"] for c in tile}
            assert {4, src["IPT_CH"] - 4, src["IPT_CH"], src["IPT_CH"] + 4, 2 * src["IPT_CH"] + 4} <= C
            for edge in (src["IPT_PTS"], src["IPT_PTS"] + 1):                            # vector and scalar stores at every C
                assert {c["C"] for c in tile if s_of(c) == edge} >= {4, src["IPT_CH"] - 4, src["IPT_CH"], src["IPT_CH"] + 4}
            _neighbours(src["CL_TILE"], {n_of(c) for c in tile}, op + " channels-last copy")
            assert 1 in {n_of(c) for c in tile}
            slices = {c["B"] * -(-c["C"] // src["IPT_CH"]) for c in tile}
            _neighbours(src["XCDS"], slices, op + " slices")
            assert {1, 2 * src["XCDS"] + 1} <= slices
            fb = [c for c in cases if c["op"] == op and GE.form(c) not in ("tile", "lane") and c.get("fmad", 0) == fmad]
            assert any(c["C"] % 4 for c in fb) and {c["ws"] for c in fb} >= {"null", "short", "misaligned"}
    assert any(c["mis"].get("out") for c in cases if c["op"] == "group_ws" and GE.form(c) != "tile")
    # plain interpolation
    for fmad in (0, 1):
        plain = [c for c in cases if c["op"] == "interp" and c["fmad"] == fmad]
        _neighbours(src["IP_THREADS"], {c["N1"] for c in plain}, "interpolation lanes")
        _neighbours(src["IP_CG"], {c["C"] for c in plain}, "interpolation channel group")
        assert {1, 2 * src["IP_CG"] + 1} <= {c["C"] for c in plain} and {1, 3} <= {c["N2"] for c in plain}
        lane = [c for c in cases if c["op"] == "interp_ws" and GE.form(c) == "lane" and c["fmad"] == fmad]
        quads = {c["C"] // 4 for c in lane if c["mode"] == "lane"}
        _neighbours(src["IPQ"], quads, "lane form quads")
        assert {1, 2 * src["IPQ"] + 1} <= quads
        _neighbours(src["IP_THREADS"], {c["N1"] for c in lane if c["mode"] == "lane"}, "lane form lanes")
        assert any(c["mode"] is None and c["mis"].get("out") for c in lane)              # reached without the knob
    # interp_add_cl: lanes per row around every divisor edge, rows around R
    lpr = {c["C"] // 4 for c in cases if c["op"] == "interp_add"}
    assert {1, 2, 3, 63, 64, 65, 128, 129, 255, 256} <= lpr and src["IA_MAX_C"] // 4 in lpr
    assert GE.IA_REFUSED_C[0] == src["IA_MAX_C"] + 4 and GE.IA_REFUSED_C[1] % 4 != 0
    for C in GE.IA_C:
        R = src["IA_ROWS"] * (src["IA_THREADS"] // (C // 4))
        assert GE.ia_rows_per_block(C) == R
        rows = {c["B"] * c["N1"] for c in cases if c["op"] == "interp_add" and c["C"] == C and c["B"] == 1}
        _neighbours(R, rows | {0}, "interp_add rows, C = %d" % C)
        assert 1 in rows
        n1 = {c["N1"] for c in cases if c["op"] == "interp_add" and c["C"] == C and c["B"] == 3}
        assert {R, R + 1} <= n1
        combos = {(c["y"], c["relu"], c["amax"]) for c in cases if c["op"] == "interp_add" and c["C"] == C}
        assert len(combos) == 8
    # both backwards
    for op in GE.BWD_OPS:
        bw = [c for c in cases if c["op"] == op]
        C = {c["C"] for c in bw}
        for T in (src["SC_CL_MIN_C"], src["SC_TILE"]):
            _neighbours(T, C, op + " channels")
        N = {c["N"] for c in bw}
        for T in (src["SC_TILE"], src["SC_THREADS"]):
            _neighbours(T, N, op + " targets")
        assert 1 in C and 1 in N
        T_ = {GE.bwd_T(c) for c in bw}
        if op == "group_bwd":
            for T in (src["SC_TILE"], src["RS_TILE"]):
                _neighbours(T, T_, op + " positions")
            assert 1 in T_
        else:
            assert {c["N1"] for c in bw} >= {1, 21, 22, 63, 64, 65, 683} and src["RS_TILE"] + 1 in T_
            assert {src["SC_TILE"] - 1, src["SC_TILE"] + 2} <= T_
        assert 0 in T_
        # the atomic kernels: a block row of GP_CG / IP_CG channels, one lane per position / per dense point
        cg, lanes = (src["GP_CG"], src["GP_THREADS"]) if op == "group_bwd" else (src["IP_CG"], src["IP_THREADS"])
        _neighbours(cg, {c["C"] for c in bw if not c["oob"]}, op + " atomic channel group")
        _neighbours(lanes, {GE.bwd_T(c) if op == "group_bwd" else c["N1"] for c in bw if not c["oob"]}, op + " atomic lanes")
        _neighbours(src["SC_THREADS"], {c["B"] * c["N"] for c in bw}, op + " keys")       # scatter_starts_kernel's lanes
        assert any(c["B"] * c["N"] == 256 and c["oob"] for c in bw)                       # a power of two, sentinel present
        assert {65535, 65536} <= {c["B"] * c["N"] for c in bw}
        assert any(c["B"] * c["N"] == 65536 and c["oob"] for c in bw) or any(c["B"] * c["N"] == 65535 and c["oob"] for c in bw)
    # the Python routing
    rg = [c for c in cases if c["op"] == "route_group"]
    for T, have in ((src["ROUTE_MIN_MK"], {mk(c) for c in rg}), (src["ROUTE_MIN_C"], {c["C"] for c in rg})):
        _neighbours(T, have, "group routing")
    assert {src["ROUTE_MIN_MK"] - 4, src["ROUTE_MIN_MK"] + 4, 3, 4, src["ROUTE_MIN_C"] - 4, src["ROUTE_MIN_C"] + 4} <= \
        {mk(c) for c in rg} | {c["C"] for c in rg}
    ri = [c for c in cases if c["op"] == "route_interp"]
    _neighbours(src["ROUTE_MIN_C"], {c["C"] for c in ri}, "interpolation routing")
    _neighbours(GE.ROUTE_N2, {c["N1"] for c in ri}, "N1 >= N2")
    assert any(c["B"] == 0 for c in rg) and any(c["B"] == 0 for c in ri)
    for c in rg:
        assert c["entry"] == GE.group_route(c["B"], c["C"], mk(c), src["ROUTE_MIN_MK"], src["ROUTE_MIN_C"])
    for c in ri:
        assert c["entry"] == GE.interp_route(c["B"], c["C"], c["N2"], c["N1"], src["ROUTE_MIN_C"])
    assert {c["entry"] for c in rg} == {"s4g_group_points_xyz_f32", "s4g_group_points_ws_f32", "s4g_group_points_f32"}
    assert {c["entry"] for c in ri} == {"s4g_three_interpolate_ws_f32", "s4g_three_interpolate_f32"}


def test_case_ids_are_unique_and_cases_are_small(cases):
    ids = [GE.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:5]
    for c in cases:
        inp = GE.inputs(c)
        assert sum(v.size for v in inp.values() if v is not None) <= 400000, GE.case_id(c)


def test_inputs_show_a_wiring_error(cases):
    for c in cases:
        for family in ("normal", "exact"):
            inp = GE.inputs(c, family)
            B = c["B"]
            if B == 0:
                continue
            N = c["N2"] if "N2" in c else c["N"]
            ix = inp["idx"].reshape(B, -1).astype(np.int64)
            T = ix.shape[1]
            inside = (ix >= 0) & (ix < N)
            assert inside.all() == (not c.get("oob") or not GE.oob_positions(T)), GE.case_id(c)
            for b in range(B):
                have = set(ix[b][inside[b]].tolist())
                if T >= 2:
                    assert {0, N - 1} <= have, GE.case_id(c)
                elif T == 1:
                    assert have <= {0, N - 1} and have
                if T >= 2 and N > 1:
                    assert ix[b, T - 1] != ix[b, T - 2], GE.case_id(c)
                if b and T >= 1 and N > 1:
                    assert not np.array_equal(ix[b], ix[b - 1]), GE.case_id(c)
            if "w" in inp:
                w = inp["w"]
                assert (w[..., 0] != w[..., 1]).all() and (w[..., 1] != w[..., 2]).all() and (w[..., 0] != w[..., 2]).all()
                if family == "exact":
                    assert np.isin(w, GE.EXACT_WEIGHTS).all()
            for k in ("feat", "gout", "sp", "y", "bias"):
                v = inp.get(k)
                if v is None:
                    continue
                assert v.dtype == np.float32
                if family == "exact":
                    assert (np.abs(v) <= GE.EXACT_MAX).all() and (v == np.round(v)).all()
    c = next(c for c in cases if c["op"] == "group_bwd" and c["oob"] and GE.bwd_T(c) >= 8)
    ix = GE.inputs(c)["idx"].reshape(c["B"], -1)
    assert {-3, c["N"], 2 ** 40} <= set(ix[0].tolist())


@pytest.mark.parametrize("family", ["normal", "exact"])
def test_restatements_are_the_oracle_bit_for_bit(oracle, cases, family):
    n = 0
    for c in cases:
        inp = GE.inputs(c, family)
        want = GE.oracle_reference(oracle, c, inp)
        if want is None:
            continue
        got = GE.reference(c, inp)
        assert got.dtype == np.float32 and got.shape == want.shape, GE.case_id(c)
        assert _bits(got) == _bits(want), GE.case_id(c)
        n += 1
    assert n == len([c for c in cases if c["op"] != "interp_add"])


def test_every_sabotage_changes_a_listed_case(cases):
    assert len(GE.SABOTAGES) >= 12
    by_op = {}
    for c in cases:
        by_op.setdefault(c["op"], []).append(c)
    clean = {}
    for name, (ops, what) in GE.SABOTAGES.items():
        seen = []
        total = 0
        for op in ops:
            for c in by_op[op]:
                cid = GE.case_id(c)
                inp = GE.inputs(c)
                if cid not in clean:
                    clean[cid] = _bits(GE.reference(c, inp))
                total += 1
                if _bits(GE.reference(c, inp, sab=name)) != clean[cid]:
                    seen.append(cid)
        print("%-16s %-90s seen by %4d of %4d cases, first %s" % (name, what, len(seen), total, seen[:1]))
        assert seen, "no case sees the sabotage %r (%s): a case is missing" % (name, what)
        for op in ops:                                                      # ... and by every operator it applies to
            assert any(s.split("-")[0] == op for s in seen), (name, op)


def test_exact_family_is_exact(cases):
    """fp32 in the kernel's order, fp32 as an fma chain, fp32 in descending order and float64 all agree bit for bit on
    the exact inputs: any summation order of an atomic backward gives these bits too."""
    for c in cases:
        if c["op"] in GE.GROUP_OPS or c["op"] == "route_group":
            continue
        inp = GE.inputs(c, "exact")
        want = GE.reference(c, inp, f64=True)
        got = GE.reference(c, inp)
        assert got.dtype == np.float32 and want.dtype == np.float64
        assert np.array_equal(got.astype(np.float64), want), GE.case_id(c)
        assert np.abs(want).max(initial=0) < 2 ** 22
        if c["op"] in GE.INTERP_OPS:
            other = GE.reference(dict(c, fmad=1 - c["fmad"]), inp)
            assert _bits(other) == _bits(got), GE.case_id(c)
        if c["op"] in GE.BWD_OPS:
            assert _bits(GE.reference(c, inp, sab="descending")) == _bits(got), GE.case_id(c)


def test_atomic_bound_holds_for_the_sequential_sum(cases):
    """The derived bound n_j 2^-23 sum |terms_j| covers the ordered fp32 sum on every case (so it is not the deterministic
    kernel's own error that sets it)."""
    for c in cases:
        if c["op"] not in GE.BWD_OPS or c["oob"]:
            continue
        inp = GE.inputs(c)
        want, bound = GE.atomic_bound(c, inp)
        got = GE.reference(c, inp).astype(np.float64)
        assert (np.abs(got - want) <= bound).all(), GE.case_id(c)
