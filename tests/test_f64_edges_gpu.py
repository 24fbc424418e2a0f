"""The operators' double dispatch (csrc/ops_f64.hip) at the edges tests/f64_edges.py lists (tests/test_f64_edges.py keeps
that list honest against the source).  Every case runs through functions.py and through the C ABI directly:
  * through the ABI every output sits between sentinel words and the FPS workspace between bytes of 0x5A, checked after
    the call; coordinates, features and gradients sit inside a NaN-filled allocation, so a read past a row shows as a
    changed result, not as a fault;
  * indices, counts, the bit patterns of the squared distances and of every gathered or interpolated value are compared
    bit for bit (NaNs by position) with the float64 numpy model AND with the C oracle's double build, under the strict
    and the fmad contract; every forward runs twice; every scene of the B = 3 run equals its own B = 1 run.
There is no tolerance in this module except the derived bound of the atomic backwards on the natural family and the
existing rtol = 1e-15 of interp_weights."""
import functools

import numpy as np
import pytest
import torch

from tests import f64_edges as FE
from tests.test_gather_edges_gpu import SENTINEL, _Out, _stream, _Ws

pytestmark = pytest.mark.gpu

CASES = {FE.case_id(c): c for c in FE.all_cases()}
PAD = 32                         # doubles either side of an input


def _ids(op):
    ops = op if isinstance(op, tuple) else (op,)
    return [i for i, c in CASES.items() if c["op"] in ops]


@pytest.fixture(autouse=True)
def _double_oracle(oracle):
    with oracle.double_dispatch():
        yield


@pytest.fixture(scope="module")
def F():
    from s4g_release_amd import functions
    functions.set_distance_mode("strict")
    return functions


class _mode:
    """functions.py's distance contract for the block."""

    def __init__(self, F, fmad):
        self.F, self.fmad = F, fmad

    def __enter__(self):
        self.F.set_distance_mode("fmad" if self.fmad else "strict")

    def __exit__(self, *exc):
        self.F.set_distance_mode("strict")
        return False


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _In:
    """A float64 input inside a NaN-filled allocation, an int64 one inside zeros."""

    def __init__(self, a, dev):
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float64, np.int64)
        flat = torch.from_numpy(a.reshape(-1))
        fill = float("nan") if a.dtype == np.float64 else 0
        self.buf = torch.full((flat.numel() + 2 * PAD,), fill, dtype=flat.dtype, device=dev)
        self.buf[PAD:PAD + flat.numel()] = flat.to(dev)
        self.ptr = self.buf.data_ptr() + PAD * 8


def _out(n, dev):
    """`n` 8-byte words between two sentinel guards."""
    return _Out(2 * n, dev)


def _flags(fmad):
    from s4g_release_amd import _cabi
    return _cabi.S4G_FLAG_FMAD if fmad else 0


def _lib():
    from s4g_release_amd import _cabi
    return _cabi.lib()


def _done(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)


# ------------------------------------------------------------------------------------------------------ ABI runners
def abi_fps(pts, M, fmad, dev, what):
    nb, _, N = pts.shape
    x, out, ws = _In(pts, dev), _out(nb * M, dev), _Ws(8 * nb * N, dev)
    _done(_lib().s4g_fps_f64(x.ptr, nb, N, M, out.ptr, ws.ptr, 8 * nb * N, _flags(fmad), _stream()), what)
    ws.check(what)
    return out.bits(what).view(np.int64).reshape(nb, M)


def abi_ball_query(pts, ctr, r, K, fmad, dev, what):
    nb, _, N = pts.shape
    M = ctr.shape[2]
    x, c, idx, cnt = _In(pts, dev), _In(ctr, dev), _out(nb * M * K, dev), _out(nb * M, dev)
    _done(_lib().s4g_ball_query_f64(x.ptr, c.ptr, nb, N, M, r, K, idx.ptr, cnt.ptr, _flags(fmad), _stream()), what)
    return idx.bits(what).view(np.int64).reshape(nb, M, K), cnt.bits(what + " (count)").view(np.int64).reshape(nb, M)


def abi_three_nn(q, k, fmad, dev, what):
    nb, _, N1 = q.shape
    N2 = k.shape[2]
    a, b, idx, d2 = _In(q, dev), _In(k, dev), _out(nb * N1 * 3, dev), _out(nb * N1 * 3, dev)
    _done(_lib().s4g_three_nn_f64(a.ptr, b.ptr, nb, N1, N2, idx.ptr, d2.ptr, _flags(fmad), _stream()), what)
    return idx.bits(what).view(np.int64).reshape(nb, N1, 3), d2.bits(what + " (d2)").view(np.float64).reshape(nb, N1, 3)


def abi_ew(c, inp, dev, what):
    """group / gather (K = 1) / interp / group_bwd / interp_bwd through the ABI -> the float64 result."""
    L = _lib()
    op, C, N = c["op"], c["C"], c["N"]
    idx = _In(inp["idx"], dev)
    nb = inp["idx"].shape[0]
    if op in ("group", "gather", "group_bwd"):
        M, K = FE.mk_of(c)
        if op == "group_bwd":
            g, gin = _In(inp["gout"], dev), _out(nb * C * N, dev)
            _done(L.s4g_group_points_backward_f64(g.ptr, idx.ptr, nb, C, N, M, K, gin.ptr, _stream()), what)
            return gin.bits(what).view(np.float64).reshape(nb, C, N)
        f, out = _In(inp["feat"], dev), _out(nb * C * M * K, dev)
        _done(L.s4g_group_points_f64(f.ptr, idx.ptr, nb, C, N, M, K, out.ptr, _stream()), what)
        return out.bits(what).view(np.float64).reshape((nb, C, M) if op == "gather" else (nb, C, M, K))
    S = c["S"]
    w = _In(inp["w"], dev)
    if op == "interp_bwd":
        g, gin = _In(inp["gout"], dev), _out(nb * C * N, dev)
        _done(L.s4g_three_interpolate_backward_f64(g.ptr, idx.ptr, w.ptr, nb, C, N, S, gin.ptr, _stream()), what)
        return gin.bits(what).view(np.float64).reshape(nb, C, N)
    f, out = _In(inp["feat"], dev), _out(nb * C * S, dev)
    _done(L.s4g_three_interpolate_f64(f.ptr, idx.ptr, w.ptr, nb, C, N, S, out.ptr, _flags(c["fmad"]), _stream()), what)
    return out.bits(what).view(np.float64).reshape(nb, C, S)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("cid", _ids("fps"))
def test_fps_edges(F, oracle, dev, cid):
    c = CASES[cid]
    pts, M, fmad = FE.fps_inputs(c), c["M"], c["fmad"]
    want = FE.fps_np(pts, M, fmad)
    assert np.array_equal(want, oracle.fps(pts, M, fmad=fmad))
    got = abi_fps(pts, M, fmad, dev, cid)
    assert np.array_equal(got, want), cid
    assert np.array_equal(abi_fps(pts, M, fmad, dev, cid), got), "run to run"
    with _mode(F, fmad):
        x = _t(pts, dev)
        through = F.farthest_point_sample(x, M)
        assert through.dtype == torch.int64 and np.array_equal(_np(through), want)
        for b in range(FE.B):
            assert np.array_equal(_np(F.farthest_point_sample(x[b:b + 1], M)), want[b:b + 1]), "scene %d alone" % b


@pytest.mark.parametrize("cid", _ids("bq"))
def test_ball_query_edges(F, oracle, dev, cid):
    c = CASES[cid]
    pts, ctr, r = FE.bq_inputs(c)
    K, fmad = c["K"], c["fmad"]
    widx, wcnt = FE.ball_query_np(pts, ctr, r, K, fmad)
    oi, oc = oracle.ball_query(pts, ctr, r, K, fmad=fmad)
    assert np.array_equal(widx, oi) and np.array_equal(wcnt, oc)
    idx, cnt = abi_ball_query(pts, ctr, r, K, fmad, dev, cid)
    assert np.array_equal(cnt, wcnt) and np.array_equal(idx, widx), cid
    again = abi_ball_query(pts, ctr, r, K, fmad, dev, cid)
    assert np.array_equal(again[0], idx) and np.array_equal(again[1], cnt), "run to run"
    with _mode(F, fmad):
        x, y = _t(pts, dev), _t(ctr, dev)
        i2, c2, g2 = F.query_and_group(x, y, r, K)
        assert np.array_equal(_np(i2), widx) and np.array_equal(_np(c2), wcnt) and g2.dtype == torch.float64
        assert FE.same(_np(g2), FE.group_points_np(pts, widx))
        for b in range(FE.B):
            ib, cb = F.ball_query(x[b:b + 1], y[b:b + 1], r, K)
            assert np.array_equal(_np(ib), widx[b:b + 1]) and np.array_equal(_np(cb), wcnt[b:b + 1]), "scene %d alone" % b


@pytest.mark.parametrize("cid", _ids("nn"))
def test_three_nn_edges(F, oracle, dev, cid):
    c = CASES[cid]
    q, k = FE.nn_inputs(c)
    fmad = c["fmad"]
    widx, wd2 = FE.three_nn_np(q, k, fmad)
    oi, od = oracle.three_nn(q, k, fmad=fmad)
    assert np.array_equal(widx, np.where(oi < 0, 0, oi)) and FE.same(wd2, od)            # index 0 in place of -1
    idx, d2 = abi_three_nn(q, k, fmad, dev, cid)
    assert np.array_equal(idx, widx) and FE.same(d2, wd2), cid
    again = abi_three_nn(q, k, fmad, dev, cid)
    assert np.array_equal(again[0], idx) and FE.same(again[1], d2), "run to run"
    with _mode(F, fmad):
        x, y = _t(q, dev), _t(k, dev)
        i2, e2 = F.search_nn_distance(x, y, 3)
        assert e2.dtype == torch.float64 and np.array_equal(_np(i2), widx) and FE.same(_np(e2), wd2)
        for b in range(FE.B):
            ib, eb = F.search_nn_distance(x[b:b + 1], y[b:b + 1], 3)
            assert np.array_equal(_np(ib), widx[b:b + 1]) and FE.same(_np(eb), wd2[b:b + 1]), "scene %d alone" % b
        w = F.interp_weights(e2)
    finite = np.isfinite(wd2).all(axis=2)
    assert np.allclose(_np(w)[finite], oracle.interp_weights(wd2)[finite], rtol=1e-15, atol=0)
    # the indices are safe to interpolate with: row 0 where the reference would have said -1
    feat = np.random.default_rng(1).standard_normal((FE.B, 2, k.shape[2]))
    ww = FE.interp_weights_np(wd2)
    with _mode(F, fmad):
        out = F.feature_interpolate(_t(feat, dev), i2, _t(ww, dev))
    assert FE.same(_np(out), FE.three_interpolate_np(feat, widx, ww, fmad))


@pytest.mark.parametrize("cid", _ids(("group", "gather", "interp")))
def test_gather_and_interpolate_edges(F, oracle, dev, cid):
    c = CASES[cid]
    op = c["op"]
    for family in ("exact", "natural"):
        inp = FE.ew_inputs(c, family)
        want = FE.ew_model(c, inp)
        assert FE.same(want, FE.ew_oracle(oracle, c, inp))
        got = abi_ew(c, inp, dev, cid)
        assert FE.same(got, want), (cid, family)
        assert FE.same(abi_ew(c, inp, dev, cid), got), "run to run"
        t = {k: _t(v, dev) for k, v in inp.items()}
        call = {"group": lambda d: F.group_points(d["feat"], d["idx"]),
                "gather": lambda d: F.gather_points(d["feat"], d["idx"]),
                "interp": lambda d: F.feature_interpolate(d["feat"], d["idx"], d["w"])}[op]
        with _mode(F, c["fmad"]):
            through = call(t)
            assert through.dtype == torch.float64 and FE.same(_np(through), want), (cid, family)
            for b in range(FE.B):
                assert FE.same(_np(call({k: v[b:b + 1] for k, v in t.items()})), want[b:b + 1]), "scene %d alone" % b


# ------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("cid", _ids(("group_bwd", "interp_bwd")))
def test_backward_edges(F, oracle, dev, cid, capsys):
    """Exact family: bit-identical to the model and the oracle (every order of addition gives the same double), through
    the ABI and through autograd.  Natural family: within n_j 2^-53 sum |terms_j| of the long-double sum per target;
    targets nobody points at are +0.0."""
    c = CASES[cid]
    op, N = c["op"], c["N"]
    inp = FE.ew_inputs(c, "exact")
    want = FE.ew_model(c, inp)
    assert FE.same(want, FE.ew_oracle(oracle, c, inp))
    got = abi_ew(c, inp, dev, cid)
    assert FE.same(got, want), cid
    t = {k: _t(v, dev) for k, v in inp.items()}
    x = torch.zeros((FE.B, c["C"], N), dtype=torch.float64, device=dev, requires_grad=True)
    out = F.group_points(x, t["idx"]) if op == "group_bwd" else F.feature_interpolate(x, t["idx"], t["w"])
    out.backward(t["gout"])
    assert x.grad.dtype == torch.float64 and FE.same(_np(x.grad), want)
    for b in range(FE.B):
        one = abi_ew(c, FE.scene(inp, b), dev, cid)
        assert FE.same(one, want[b:b + 1]), "scene %d alone" % b
    inp = FE.ew_inputs(c, "natural")
    got = abi_ew(c, inp, dev, cid)
    ref, bound = FE.atomic_bound(c, inp)
    err = np.abs(got.astype(np.longdouble) - ref)
    assert (got[np.asarray(bound == 0)] == 0).all() and not np.signbit(got[np.asarray(bound == 0)]).any()
    frac = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    with capsys.disabled():
        print("\n%s: atomic error at %.3g of the bound" % (cid, frac))
    assert (err <= bound).all(), (cid, frac)


# ------------------------------------------------------------------------------------------------------ refusals
BIG = 1 << 20                    # words per buffer: room for B = 65 536 or C = 65 536 beside the other base sizes
BASE = dict(B=2, C=2, N=4, M=2, K=2, N1=4, N2=4)
E, W, OK = "EINVAL", "EWORKSPACE", "OK"
P31, P23 = 1 << 31, 1 << 23
COMMON = [({"B": -1}, E), ({"B": 65536}, E), ({"B": 0}, OK)]
GROUP_SIZES = [({"C": -1}, E), ({"N": 0}, E), ({"M": -1}, E), ({"K": -1}, E), ({"C": 65536}, E), ({"N": P31}, E)]
INTERP_SIZES = [({"C": -1}, E), ({"N2": 0}, E), ({"N1": -1}, E), ({"C": 65536}, E), ({"N1": P31}, E)]
# entry point -> (argument names in ABI order, outputs, [(what differs from BASE, expected)]); "zero" says the output
# is zero-filled instead of untouched
REFUSALS = {
    "s4g_fps_f64": (("xyz", "B", "N", "M", "idx", "ws", "ws_bytes", "flags"), ("idx",), COMMON + [
        ({"N": 0}, E), ({"M": 0}, E), ({"M": 5}, E), ({"N": P23, "M": 1}, E), ({"xyz": None}, E), ({"idx": None}, E),
        ({"ws": None}, W), ({"ws_bytes": 8 * 2 * 4 - 1}, W), ({"ws_bytes": 0}, W)]),
    "s4g_ball_query_f64": (("xyz", "ctr", "B", "N", "M", "radius", "K", "idx", "cnt", "flags"), ("idx", "cnt"), COMMON + [
        ({"N": 0}, E), ({"M": -1}, E), ({"K": 0}, E), ({"N": P31}, E), ({"M": 0}, OK), ({"xyz": None}, E),
        ({"ctr": None}, E), ({"idx": None}, E), ({"cnt": None}, E)]),
    "s4g_three_nn_f64": (("q", "k", "B", "N1", "N2", "idx", "d2", "flags"), ("idx", "d2"), COMMON + [
        ({"N1": -1}, E), ({"N2": 2}, E), ({"N1": P31}, E), ({"N2": P31}, E), ({"N1": 0}, OK), ({"q": None}, E),
        ({"k": None}, E), ({"idx": None}, E), ({"d2": None}, E)]),
    "s4g_group_points_f64": (("feat", "gidx", "B", "C", "N", "M", "K", "out"), ("out",), COMMON + GROUP_SIZES + [
        ({"C": 0}, OK), ({"M": 0}, OK), ({"K": 0}, OK), ({"feat": None}, E), ({"gidx": None}, E), ({"out": None}, E)]),
    "s4g_group_points_backward_f64": (("gout", "gidx", "B", "C", "N", "M", "K", "gin"), ("gin",), COMMON + GROUP_SIZES + [
        ({"C": 0}, OK), ({"M": 0}, "zero"), ({"K": 0}, "zero"), ({"M": 0, "gout": None, "gidx": None}, "zero"),
        ({"gout": None}, E), ({"gidx": None}, E), ({"gin": None}, E)]),
    "s4g_three_interpolate_f64": (("feat", "nidx", "w", "B", "C", "N2", "N1", "out", "flags"), ("out",),
                                  COMMON + INTERP_SIZES + [
        ({"C": 0}, OK), ({"N1": 0}, OK), ({"feat": None}, E), ({"nidx": None}, E), ({"w": None}, E), ({"out": None}, E)]),
    "s4g_three_interpolate_backward_f64": (("gout", "nidx", "w", "B", "C", "N2", "N1", "gin"), ("gin",),
                                           COMMON + INTERP_SIZES + [
        ({"C": 0}, OK), ({"N1": 0}, "zero"), ({"N1": 0, "gout": None, "nidx": None, "w": None}, "zero"),
        ({"gout": None}, E), ({"nidx": None}, E), ({"w": None}, E), ({"gin": None}, E)]),
}
REFUSAL_IDS = [(name, i) for name, (_, _, rows) in REFUSALS.items() for i in range(len(rows))]


@functools.lru_cache(maxsize=None)
def _refusal_buffers(dev):
    """One set of BIG-word buffers for every refusal: valid inputs of the BASE sizes at their start, zeros behind."""
    rng = np.random.default_rng(5)
    f = lambda: torch.from_numpy(np.concatenate([rng.random(4096), np.zeros(BIG - 4096)])).to(dev)
    z = lambda: torch.zeros(BIG, dtype=torch.int64, device=dev)
    return dict(xyz=f(), ctr=f(), q=f(), k=f(), feat=f(), gout=f(), w=f(), gidx=z(), nidx=z(),
                ws=torch.zeros(BIG, dtype=torch.float64, device=dev))


@pytest.mark.parametrize("name,row", REFUSAL_IDS, ids=lambda v: str(v))
def test_refusals(dev, name, row):
    """Every condition an entry point's first lines test: S4G_EINVAL / S4G_EWORKSPACE and the sentinel-filled outputs
    untouched; an empty problem (B, M, N1, C or M K of 0) S4G_OK and untouched; the two backwards with nothing to
    scatter zero-fill gin.  (Every buffer is large enough for the sizes the call names wherever the call is not refused
    before its first launch by the lines above it -- B or C of 65 536 among them -- and N >= 2^31, 2^23 only name sizes:
    they are refused before anything is started.)"""
    from s4g_release_amd import _cabi
    names, outs, rows = REFUSALS[name]
    diff, expect = rows[row]
    bufs = _refusal_buffers(dev)
    fill = torch.iinfo(torch.int64).min + 12345
    out_bufs = {o: torch.full((BIG,), fill, dtype=torch.int64, device=dev) for o in outs}
    vals = dict(BASE, radius=0.25, flags=0, ws_bytes=8 * BASE["B"] * BASE["N"])
    vals.update({k: v.data_ptr() for k, v in bufs.items()})
    vals.update({k: v.data_ptr() for k, v in out_bufs.items()})
    vals.update(diff)
    rc = getattr(_cabi.lib(), name)(*[vals[n] for n in names], _stream())
    torch.cuda.synchronize()
    assert rc == {E: _cabi.S4G_EINVAL, W: _cabi.S4G_EWORKSPACE, OK: 0, "zero": 0}[expect], (name, diff, rc)
    for o, buf in out_bufs.items():
        if expect == "zero":
            n = BASE["B"] * BASE["C"] * (BASE["N"] if "group" in name else BASE["N2"])
            assert (buf[:n] == 0).all() and (buf[n:] == fill).all(), (name, diff)
        else:
            assert (buf == fill).all(), (name, diff, o)


def test_base_sizes_of_the_refusals_are_accepted(dev):
    """The same calls without a difference succeed: the refusals above are owed to the one thing each changes."""
    from s4g_release_amd import _cabi
    bufs = _refusal_buffers(dev)
    for name, (names, outs, _) in REFUSALS.items():
        out_bufs = {o: torch.full((BIG,), -7, dtype=torch.int64, device=dev) for o in outs}
        vals = dict(BASE, radius=0.25, flags=0, ws_bytes=8 * BASE["B"] * BASE["N"])
        vals.update({k: v.data_ptr() for k, v in bufs.items()})
        vals.update({k: v.data_ptr() for k, v in out_bufs.items()})
        rc = getattr(_cabi.lib(), name)(*[vals[n] for n in names], _stream())
        torch.cuda.synchronize()
        assert rc == 0, name
        assert all((b[:2] != -7).any() for b in out_bufs.values()), name


def test_wrappers_refuse_float_double_mixes(F, dev):
    """Every operator with two floating-point arguments, both ways round; a float call next to them is untouched."""
    rng = np.random.default_rng(3)
    d = lambda *s: _t(rng.random(s), dev)
    f = lambda *s: d(*s).float()
    idx3 = torch.zeros((1, 8, 3), dtype=torch.int64, device=dev)
    mixes = [
        lambda: F.ball_query(d(1, 3, 20), f(1, 3, 4), 0.3, 4), lambda: F.ball_query(f(1, 3, 20), d(1, 3, 4), 0.3, 4),
        lambda: F.query_and_group(d(1, 3, 20), f(1, 3, 4), 0.3, 4), lambda: F.query_and_group(f(1, 3, 20), d(1, 3, 4), 0.3, 4),
        lambda: F.search_nn_distance(d(1, 3, 8), f(1, 3, 5), 3), lambda: F.search_nn_distance(f(1, 3, 8), d(1, 3, 5), 3),
        lambda: F.feature_interpolate(d(1, 2, 5), idx3, f(1, 8, 3)), lambda: F.feature_interpolate(f(1, 2, 5), idx3, d(1, 8, 3)),
        lambda: F._interpolate_backward(d(1, 2, 8), idx3, f(1, 8, 3), 5), lambda: F._interpolate_backward(f(1, 2, 8), idx3, d(1, 8, 3), 5),
    ]
    for n, call in enumerate(mixes):
        with pytest.raises(RuntimeError, match="share one dtype"):
            call()
    # one floating-point argument: the dtype decides, nothing to mix
    i2 = torch.zeros((1, 4, 2), dtype=torch.int64, device=dev)
    for make, dt in ((d, torch.float64), (f, torch.float32)):
        assert F.farthest_point_sample(make(1, 3, 20), 5).dtype == torch.int64
        assert F.group_points(make(1, 2, 5), i2).dtype == dt and F.gather_points(make(1, 2, 5), i2[:, :, 0]).dtype == dt
        assert F._group_points_backward(make(1, 2, 4, 2), i2, 5).dtype == dt
        assert F.interp_weights(make(1, 8, 3)).dtype == dt
