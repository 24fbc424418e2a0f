"""group_points, gather_points, three_interpolate (plain, tile and lane forms), interp_add_cl and both backwards at the
edges tests/gather_edges.py lists (tests/test_gather_edges.py keeps that list honest against the sources).  Every case
calls the C ABI directly:
  * every output sits between 64 sentinel words, every workspace between 256 bytes of 0x5A, checked after the call; the
    guarded view starts 16-byte aligned unless the case offsets it on purpose;
  * features and gradients sit inside a NaN-filled allocation: a read one row or one quad outside shows as a NaN in the
    output, not as a fault;
  * forward results, every fallback and the deterministic backward are compared bit for bit with the CPU oracle (with the
    fp32 numpy restatement for interp_add_cl, which the oracle does not have), and run twice.
There is no tolerance in this module except the derived bound of the atomic backwards on normal gradients."""
import numpy as np
import pytest
import torch

from tests import gather_edges as GE

pytestmark = pytest.mark.gpu

GUARD = 64                      # words either side of an output, of an input
SENTINEL = -559038737
WS_GUARD = 256                  # bytes either side of a workspace
WS_BYTE = 0x5A


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Out:
    """`n` 4-byte words between two guards; the view starts `off` bytes past a 16-byte boundary."""

    def __init__(self, n, dev, off=0, fill=SENTINEL):
        assert off % 4 == 0 and 0 <= off < 16
        self.buf = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.int32, device=dev)
        self.lo, self.n = GUARD + off // 4, n
        self.view = self.buf[self.lo:self.lo + n]
        if fill != SENTINEL:
            self.view.fill_(fill)
        assert self.buf.data_ptr() % 256 == 0 and self.view.data_ptr() % 16 == off

    @property
    def ptr(self):
        return self.view.data_ptr()

    def bits(self, what):
        """The words as int32, after the guards were found intact."""
        assert (self.buf[:self.lo] == SENTINEL).all() and (self.buf[self.lo + self.n:] == SENTINEL).all(), \
            "guard of %s" % what
        return self.view.cpu().numpy().copy()


class _Ws:
    def __init__(self, nbytes, dev, off=0):
        self.buf = torch.full((nbytes + 2 * WS_GUARD + 16,), WS_BYTE, dtype=torch.uint8, device=dev)
        self.lo, self.n = WS_GUARD + off, nbytes
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + self.lo
        assert self.ptr % 16 == off % 16

    def check(self, what):
        assert (self.buf[:self.lo] == WS_BYTE).all() and (self.buf[self.lo + self.n:] == WS_BYTE).all(), \
            "guard of the workspace of %s" % what

    def touched(self, start=0):
        """Whether anything was written from byte `start` of the workspace on."""
        return bool((self.buf[self.lo + start:self.lo + self.n] != WS_BYTE).any().item())


class _In:
    """A float32 input inside a NaN-filled allocation, or an index inside zeros (`off` bytes past 16-byte alignment)."""

    def __init__(self, a, dev, off=0):
        a = np.ascontiguousarray(a)
        flat = torch.from_numpy(a.reshape(-1))
        step = a.dtype.itemsize
        assert off % step == 0
        pad = 256 // step
        if a.dtype == np.float32:
            self.buf = torch.full((flat.numel() + 2 * pad + 4,), float("nan"), dtype=torch.float32, device=dev)
        else:
            self.buf = torch.zeros((flat.numel() + 2 * pad + 4,), dtype=flat.dtype, device=dev)
        lo = pad + off // step
        self.buf[lo:lo + flat.numel()] = flat.to(dev)
        self.ptr = self.buf.data_ptr() + lo * step
        assert self.buf.data_ptr() % 256 == 0 and self.ptr % 16 == off


def _f32(bits):
    return bits.view(np.float32)


def _same(got_bits, want, what):
    want = np.ascontiguousarray(want, dtype=np.float32).reshape(-1).view(np.int32)
    bad = np.nonzero(got_bits != want)[0]
    assert len(bad) == 0, "%s: %d of %d words differ, first at %d: got %r want %r" % (
        what, len(bad), len(want), bad[0], _f32(got_bits)[bad[0]], want.view(np.float32)[bad[0]])


def _workspace(c, nbytes, dev):
    """-> (_Ws or None, pointer, byte count) for the case's workspace kind."""
    kind = c["ws"]
    if kind == "null":
        return None, None, 0
    short = {"group_xyz": 16}.get(c["op"], 4) if kind == "short" else 0
    ws = _Ws(nbytes - short, dev, off=8 if kind == "misaligned" else 0)
    return ws, ws.ptr, nbytes - short


# ------------------------------------------------------------------------------------------------------ forward
def _run_forward(c, inp, dev, monkeypatch):
    """One call of the case's entry point -> the output's words.  The workspace is written exactly where a form that
    needs it answered (the index-ordered copy of the xyz form, the channels-last copy of the tile and lane forms): that
    is how a fallback shows through the ABI."""
    from s4g_release_amd import _cabi
    L = _cabi.lib()
    op, B, C, mis = c["op"], c["B"], c["C"], c["mis"]
    feat = _In(inp["feat"], dev)
    idx = _In(inp["idx"], dev, off=mis.get("idx", 0))
    if op in GE.GROUP_OPS:
        N, M, K = c["N"], c["M"], c["K"]
        out = _Out(B * C * M * K, dev, off=mis.get("out", 0))
        ws = None
        if op == "gather":
            rc = L.s4g_gather_points_f32(feat.ptr, idx.ptr, B, C, N, M, out.ptr, _stream())
        elif op == "group":
            rc = L.s4g_group_points_f32(feat.ptr, idx.ptr, B, C, N, M, K, out.ptr, _stream())
        elif op == "group_xyz":
            ws, p, nb = _workspace(c, B * N * 16, dev)
            rc = L.s4g_group_points_xyz_f32(feat.ptr, idx.ptr, B, N, M, K, out.ptr, p, nb, _stream())
        else:
            ws, p, nb = _workspace(c, B * N * C * 4, dev)
            rc = L.s4g_group_points_ws_f32(feat.ptr, idx.ptr, B, C, N, M, K, out.ptr, p, nb, _stream())
    else:
        N2, N1 = c["N2"], c["N1"]
        w = _In(inp["w"], dev)
        out = _Out(B * C * N1, dev, off=mis.get("out", 0))
        flags = _cabi.S4G_FLAG_FMAD if c["fmad"] else 0
        ws = None
        if c["mode"]:
            monkeypatch.setenv("S4G_INTERP_MODE", c["mode"])
        else:
            monkeypatch.delenv("S4G_INTERP_MODE", raising=False)
        if op == "interp":
            rc = L.s4g_three_interpolate_f32(feat.ptr, idx.ptr, w.ptr, B, C, N2, N1, out.ptr, flags, _stream())
        else:
            ws, p, nb = _workspace(c, B * N2 * C * 4, dev)
            rc = L.s4g_three_interpolate_ws_f32(feat.ptr, idx.ptr, w.ptr, B, C, N2, N1, out.ptr, p, nb, flags, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    if ws is not None:
        ws.check(GE.case_id(c))
        assert ws.touched() == (GE.form(c) in ("aos", "tile", "lane")), (GE.case_id(c), GE.form(c))
    return out.bits(GE.case_id(c))


def _replaced_form(c):
    """The case a fallback case stands in for: the same sizes with a whole, aligned workspace and aligned pointers, or
    (where the sizes themselves rule the fast form out) the plain entry point."""
    twin = dict(c, mis={}, mode=None, ws="full" if c["ws"] else None)
    if GE.form(twin) == GE.form(c) or twin == c:
        plain = {"group_xyz": "group", "group_ws": "group", "interp_ws": "interp"}.get(c["op"])
        if plain is None:
            return None
        twin = dict(twin, op=plain, ws=None)
    return twin


FORWARD = GE.group_cases() + GE.interp_cases()


@pytest.mark.parametrize("c", FORWARD, ids=GE.case_id)
def test_forward_edges(oracle, dev, monkeypatch, c):
    """Bit-identical to the oracle on both input families and from run to run; a fallback bit-identical to the form it
    replaces; all guards intact."""
    primary = {"group": "vec4", "gather": None, "group_xyz": "aos", "group_ws": "tile", "interp": "plain",
               "interp_ws": "tile"}[c["op"]]
    for family in ("normal", "exact"):
        inp = GE.inputs(c, family)
        want = GE.oracle_reference(oracle, c, inp)
        got = _run_forward(c, inp, dev, monkeypatch)
        _same(got, want, "%s (%s, %s)" % (GE.case_id(c), GE.form(c), family))
        again = _run_forward(c, inp, dev, monkeypatch)
        assert np.array_equal(got, again), "run to run"
        if family == "exact" and c["op"] in GE.INTERP_OPS:
            assert np.array_equal(_f32(got).astype(np.float64).reshape(want.shape), GE.reference(c, inp, f64=True))
        if primary is not None and GE.form(c) != primary:
            twin = _replaced_form(c)
            if twin is not None:
                other = _run_forward(twin, inp, dev, monkeypatch)
                assert np.array_equal(got, other), "fallback %s against %s" % (GE.form(c), GE.form(twin))


# ------------------------------------------------------------------------------------------------------ interp_add_cl
def _run_interp_add(c, inp, dev, expect=0):
    from s4g_release_amd import _cabi
    B, N1, N2, C = c["B"], c["N1"], c["N2"], c["C"]
    sp, idx, w, bias = _In(inp["sp"], dev), _In(inp["idx"], dev), _In(inp["w"], dev), _In(inp["bias"], dev)
    y = _In(inp["y"], dev) if inp["y"] is not None else None
    out = _Out(B * N1 * C, dev)
    amax = _Out(B * 64, dev, fill=0) if c["amax"] else None
    rc = _cabi.lib().s4g_interp_add_cl_f32(None if y is None else y.ptr, sp.ptr, idx.ptr, w.ptr, bias.ptr, B, N1, N2, C,
                                           c["relu"], out.ptr, None if amax is None else amax.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    what = GE.case_id(c)
    return out.bits(what), None if amax is None else amax.bits(what + " (out_amax)")


@pytest.mark.parametrize("B,N1,C", GE.interp_add_shapes(), ids=lambda v: str(v))
def test_interp_add_edges(dev, B, N1, C):
    """out bit-identical to the fp32 restatement in the kernel's documented order; a scene's out_amax row maximum is at
    least its own max |out|, at most the maximum over the scenes that share a workgroup with it, and exactly its own
    where N1 is a multiple of the workgroup's row count; nothing is written for a scene index >= B (the guard behind
    the (B, 64) rows)."""
    R = GE.ia_rows_per_block(C)
    cases = [c for c in GE.interp_add_cases() if (c["B"], c["N1"], c["C"]) == (B, N1, C)]
    assert len(cases) == 8
    for c in cases:
        for family in ("normal", "exact"):
            inp = GE.inputs(c, family)
            want = GE.reference(c, inp)
            got, amax = _run_interp_add(c, inp, dev)
            _same(got, want, "%s (%s)" % (GE.case_id(c), family))
            if family == "exact":
                assert np.array_equal(_f32(got).astype(np.float64).reshape(want.shape), GE.reference(c, inp, f64=True))
            again, amax2 = _run_interp_add(c, inp, dev)
            assert np.array_equal(got, again)
            if amax is None:
                continue
            own = np.abs(want.reshape(B, N1 * C)).max(axis=1)
            row = _f32(amax).reshape(B, 64).max(axis=1)
            assert np.array_equal(row, _f32(amax2).reshape(B, 64).max(axis=1))
            assert (_f32(amax) >= 0).all()
            for b in range(B):
                first, last = (b * N1) // R, ((b + 1) * N1 - 1) // R                     # the workgroups of scene b's rows
                shared = [s for s in range(B) if (s * N1) // R <= last and ((s + 1) * N1 - 1) // R >= first]
                assert own[b] <= row[b] <= max(own[s] for s in shared), (GE.case_id(c), family, b)
                if N1 % R == 0:
                    assert row[b] == own[b], (GE.case_id(c), family, b)


@pytest.mark.parametrize("C", GE.IA_REFUSED_C)
def test_interp_add_refuses(dev, C):
    """More than 1 024 channels, or a count that is no multiple of 4: S4G_EINVAL, nothing written."""
    from s4g_release_amd import _cabi
    c = dict(op="interp_add", B=2, N1=9, N2=5, C=C, y=1, relu=1, amax=1)
    got, amax = _run_interp_add(c, GE.inputs(c), dev, expect=_cabi.S4G_EINVAL)
    assert (got == SENTINEL).all() and (amax == 0).all()


# ------------------------------------------------------------------------------------------------------ backward
def _run_backward(c, inp, dev, kind):
    """-> the words of gin.  kind "cl": deterministic with the workspace s4g_scatter_det_workspace_bytes_c asks for, "plain": with the one of
    s4g_scatter_det_workspace_bytes (no room for the channels-last copy), "atomic": the atomicAdd entry point."""
    from s4g_release_amd import _cabi
    L = _cabi.lib()
    op, B, C, N = c["op"], c["B"], c["C"], c["N"]
    T = GE.bwd_T(c)
    weighted = op == "interp_bwd"
    gout = _In(inp["gout"], dev) if T else None
    idx = _In(inp["idx"], dev) if T else None
    w = _In(inp["w"], dev) if weighted and T else None
    gin = _Out(B * C * N, dev)
    ws, p, nb, plain = None, None, 0, 0
    if kind != "atomic" and T:
        plain = L.s4g_scatter_det_workspace_bytes(B, N, T)
        full = L.s4g_scatter_det_workspace_bytes_c(B, C, N, T, int(weighted))
        assert plain > 0 and (full > plain) == (C >= GE.SC_CL_MIN_C) and (full == plain) == (C < GE.SC_CL_MIN_C)
        nb = full if kind == "cl" else plain
        ws = _Ws(nb, dev)
        assert ws.ptr % 256 == 0
        p = ws.ptr
    g = lambda t: None if t is None else t.ptr
    if weighted:
        args = (g(gout), g(idx), g(w), B, C, N, c["N1"], gin.ptr)
        rc = L.s4g_three_interpolate_backward_f32(*args, _stream()) if kind == "atomic" else \
            L.s4g_three_interpolate_backward_det_f32(*args, p, nb, _stream())
    else:
        args = (g(gout), g(idx), B, C, N, c["M"], c["K"], gin.ptr)
        rc = L.s4g_group_points_backward_f32(*args, _stream()) if kind == "atomic" else \
            L.s4g_group_points_backward_det_f32(*args, p, nb, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    if ws is not None:
        ws.check(GE.case_id(c))
        # the channels-last copy of the gradients lies behind the plain workspace: written exactly where that form ran
        assert ws.touched() and ws.touched(plain) == (kind == "cl" and C >= GE.SC_CL_MIN_C), (GE.case_id(c), kind)
    return gin.bits("%s (%s)" % (GE.case_id(c), kind))


@pytest.mark.parametrize("c", GE.bwd_cases(), ids=GE.case_id)
def test_backward_edges(oracle, dev, c):
    """The deterministic backward bit-identical to the oracle from the workspace with room for the channels-last copy
    and from the one without, and from run to run; targets nobody points at +0.0 by bit pattern; out-of-range indices
    (-3, N, 2^40) count for nobody.  The atomic backward (in-range indices only) bit-identical on the exact family and
    within n_j 2^-23 sum |terms_j| of float64 per target on normal gradients."""
    B, N = c["B"], c["N"]
    for family in ("normal", "exact"):
        inp = GE.inputs(c, family)
        want = GE.oracle_reference(oracle, c, inp)
        ix = inp["idx"].reshape(B, -1)
        hit = np.zeros((B, N), bool)
        for b in range(B):
            hit[b, ix[b][(ix[b] >= 0) & (ix[b] < N)]] = True
        empty = np.broadcast_to(~hit[:, None, :], want.shape).reshape(-1)
        for kind in ("cl", "plain"):
            got = _run_backward(c, inp, dev, kind)
            _same(got, want, "%s (%s, %s)" % (GE.case_id(c), kind, family))
            assert (got[empty] == 0).all(), "untouched targets are +0.0"
            assert np.array_equal(got, _run_backward(c, inp, dev, kind)), "run to run"
        if c["oob"]:
            continue                                                       # the atomic kernels do not range-check
        got = _run_backward(c, inp, dev, "atomic")
        assert (got[empty] == 0).all()
        if family == "exact":
            _same(got, want, "%s (atomic, exact)" % GE.case_id(c))
        else:
            ref, bound = GE.atomic_bound(c, inp)
            err = np.abs(_f32(got).astype(np.float64).reshape(ref.shape) - ref)
            print("%s: atomic error at %.3g of the bound" % (GE.case_id(c), float((err / np.maximum(bound, 1e-300)).max())
                                                              if err.size else 0.0))
            assert (err <= bound).all(), (GE.case_id(c), float(err.max()))


def test_backward_workspace_one_byte_short_is_refused(dev):
    """S4G_EWORKSPACE, and nothing written, when the workspace is smaller than s4g_scatter_det_workspace_bytes says."""
    from s4g_release_amd import _cabi
    L = _cabi.lib()
    c = dict(op="group_bwd", B=2, C=33, N=65, M=16, K=4, oob=0)
    inp = GE.inputs(c)
    gout, idx, gin = _In(inp["gout"], dev), _In(inp["idx"], dev), _Out(2 * 33 * 65, dev)
    nb = L.s4g_scatter_det_workspace_bytes(2, 65, 64)
    ws = _Ws(nb, dev)
    rc = L.s4g_group_points_backward_det_f32(gout.ptr, idx.ptr, 2, 33, 65, 16, 4, gin.ptr, ws.ptr, nb - 1, _stream())
    torch.cuda.synchronize()
    assert rc == _cabi.S4G_EWORKSPACE
    assert (gin.bits("gin") == SENTINEL).all() and (ws.buf == WS_BYTE).all()


# ------------------------------------------------------------------------------------------------------ Python routing
class _RecordingLib:
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("s4g_"):
            return fn

        def call(*args):
            self._calls.append(name)
            return fn(*args)
        return call


class _RecordingCabi:
    """functions._cabi with every library call recorded by name."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def lib(self):
        return _RecordingLib(self._real.lib(), self.calls)

    def __getattr__(self, name):
        return getattr(self._real, name)


@pytest.mark.parametrize("c", GE.route_cases(), ids=GE.case_id)
def test_python_routing(oracle, dev, monkeypatch, c):
    """F.group_points / F.feature_interpolate on both sides of every routing literal: the entry point reached is the one
    the table states, and the result is the oracle's."""
    from s4g_release_amd import functions
    functions.set_distance_mode("strict")
    monkeypatch.delenv("S4G_INTERP_MODE", raising=False)
    proxy = _RecordingCabi(functions._cabi)
    monkeypatch.setattr(functions, "_cabi", proxy)
    inp = GE.inputs(c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if c["op"] == "route_group":
        got = functions.group_points(t(inp["feat"]), t(inp["idx"]))
    else:
        got = functions.feature_interpolate(t(inp["feat"]), t(inp["idx"]), t(inp["w"]))
    torch.cuda.synchronize()
    want = GE.oracle_reference(oracle, c, inp)
    ops = [n for n in proxy.calls if "group_points" in n or "three_interpolate" in n]
    assert ops == [c["entry"]], (ops, c["entry"])
    assert tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
