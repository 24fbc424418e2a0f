"""FPS, ball query and 3-NN at every kernel-dispatch boundary (tests/dispatch_edges.py lists the sizes and why;
tests/test_dispatch_edges.py keeps that list honest against the sources).  Every case runs on the same seeded input
as the CPU oracle; indices, counts, gathered coordinates, squared distances and pick distances are compared bit for
bit -- there is no tolerance and no skip in this module.

Which kernel ran is checked through what the ABI exposes, without a profiler:
  * `s4g_workspace_bytes(S4G_OP_FPS)` is non-zero up to 25 600 points exactly where a pre-pass form may run, and is
    exactly the streaming kernel's B N floats past 65 535;
  * with pick distances requested `s4g_fps_gather_ex_i32` answers S4G_EUNSUPPORTED (and writes nothing) exactly where
    the streaming kernel is the only choice;
  * the register kernel never touches the workspace it is handed, the pre-pass of the pruned and the L2 kernels and the
    streaming kernel's min-distances do: a workspace filled with a marker byte comes back changed or not.
That separates reg / pruned / pruned-L2 / stream.  It cannot tell WHICH instantiation of a form ran (<512,20> against
<512,32>, 100 against 128 slots): that follows from N by the S4G_FPS_CASE / S4G_FPS_PRUNED lists, which the CPU test
reads.  For 3-NN the routing (split scan, lane scan, grid) has no observable besides its result; the knobs that force
the other side of each boundary are driven instead, and both sides must give the oracle's answer."""
import numpy as np
import pytest
import torch

from tests import dispatch_edges as DE
from tests.test_ops_gpu import _prefix_check, _t

pytestmark = pytest.mark.gpu

MARK = 0xA5


@pytest.fixture(scope="module")
def F():
    from s4g_release_amd import functions
    functions.set_distance_mode("strict")
    return functions


def _set_fps_mode(monkeypatch, mode):
    if mode == "default":
        monkeypatch.delenv("S4G_FPS_MODE", raising=False)
    else:
        monkeypatch.setenv("S4G_FPS_MODE", mode)


class _fmad:
    """The fmad distance contract for a block (S4G_FLAG_FMAD in every call of the operator API)."""

    def __init__(self, F, on=True):
        self.F, self.on = F, on

    def __enter__(self):
        if self.on:
            self.F.set_distance_mode("fmad")

    def __exit__(self, *exc):
        self.F.set_distance_mode("strict")
        return False


def _first_diff(got, want):
    """(scene, pick, got, want) of the first differing pick, for the failure message."""
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return None
    b, k = (int(v) for v in bad[0])
    return b, k, int(got[b, k]), int(want[b, k])


def _fps_call(F, pts, M, dev, want_dist, ws_kind="full"):
    """s4g_fps_gather_ex_i32 on a marker-filled workspace -> (rc, idx int64, ctr, dist or None, workspace touched).
    ws_kind: "full" = what s4g_workspace_bytes asks for, "null" = no workspace, "short" = one byte too few."""
    from s4g_release_amd import _cabi
    B, _, N = pts.shape
    x = _t(pts, dev)
    idx = torch.full((B, M), -7, dtype=torch.int32, device=dev)
    ctr = torch.full((B, 3, M), -7.0, dtype=torch.float32, device=dev)
    dist = torch.full((B, M), -7.0, dtype=torch.float32, device=dev) if want_dist else None
    nbytes = _cabi.lib().s4g_workspace_bytes(_cabi.S4G_OP_FPS, B, N, M, 0)
    ws = torch.full((max(nbytes, 1),), MARK, dtype=torch.uint8, device=dev)
    ptr, passed = (None, 0) if ws_kind == "null" or nbytes == 0 else (ws.data_ptr(), nbytes - (ws_kind == "short"))
    rc = _cabi.lib().s4g_fps_gather_ex_i32(x.data_ptr(), B, N, M, idx.data_ptr(), ctr.data_ptr(),
                                           None if dist is None else dist.data_ptr(), None, ptr, passed,
                                           F._DIST_FLAGS, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    touched = bool((ws != MARK).any().item())
    return (rc, idx.cpu().numpy().astype(np.int64), ctr.cpu().numpy(),
            None if dist is None else dist.cpu().numpy(), touched)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_form(F, oracle, pts, M, dev, form, want, fmad=False, what=None):
    """One cloud through s4g_fps_gather_ex_i32 with pick distances: the form that answered, and everything it wrote."""
    from s4g_release_amd import _cabi
    base = form.split("<")[0]
    rc, idx, ctr, dist, touched = _fps_call(F, pts, M, dev, want_dist=True)
    if base == "stream":
        assert rc == _cabi.S4G_EUNSUPPORTED, (what, rc)
        assert (idx == -7).all() and (ctr == -7.0).all() and (dist == -7.0).all() and not touched, what
        rc, idx, ctr, _, touched = _fps_call(F, pts, M, dev, want_dist=False)
        assert rc == 0 and touched, (what, rc, touched)
    else:
        assert rc == 0, (what, rc)
        assert touched == (base != "reg"), (what, form, touched)
    assert np.array_equal(idx, want), (what, form, _first_diff(idx, want))
    assert np.array_equal(_bits(ctr), _bits(oracle.gather_points(pts, want))), what
    if base != "stream":
        for b in range(pts.shape[0]):
            D = DE.pick_distances(pts[b], want[b], fmad)
            assert np.array_equal(_bits(dist[b]), _bits(D)), (what, form, b, int(np.argmax(_bits(dist[b]) != _bits(D))))
    return ctr, dist


# ------------------------------------------------------------------------------------------------------------ FPS
@pytest.mark.parametrize("N,M,mode,form", DE.fps_cases())
def test_fps_ladder(F, oracle, dev, monkeypatch, N, M, mode, form):
    """Every (N, M, mode) of the ladder: the operator API's indices, and the int32 + centroid + pick-distance entry
    point's indices, coordinates and D_k, on two scenes each of uniform, lattice and (N > 10 240) table-top input;
    the kernel form that answered is the one the ladder states."""
    from s4g_release_amd import _cabi
    _set_fps_mode(monkeypatch, mode)
    nbytes = _cabi.lib().s4g_workspace_bytes(_cabi.S4G_OP_FPS, 2, N, M, 0)
    if N <= DE.FPS_REG_TOP:
        assert (nbytes != 0) == (mode != "dense" and N > DE.FPS_MAY_PRUNE_ABOVE[mode]), nbytes
    elif N <= DE.FPS_L2_TOP:
        assert nbytes > 2 * N * 4
    else:
        assert nbytes == 2 * N * 4
    for kind, pts in DE.fps_inputs(N, M).items():
        want = oracle.fps(pts, M)
        got = F.farthest_point_sample(_t(pts, dev), M).cpu().numpy()
        assert got.dtype == np.int64
        assert np.array_equal(got, want), (kind, form, _first_diff(got, want))
        _check_form(F, oracle, pts, M, dev, form, want, what=kind)


@pytest.mark.parametrize("N,M,mode", DE.FPS_FMAD)
def test_fps_ladder_fmad_contract(F, oracle, dev, monkeypatch, N, M, mode):
    """One size per kernel form under S4G_FLAG_FMAD, against the oracle's fmad restatement."""
    _set_fps_mode(monkeypatch, mode)
    form = {(n, m, md): f for n, m, md, f in DE.fps_cases()}[(N, M, mode)]
    for kind, pts in DE.fps_inputs(N, M).items():
        want = oracle.fps(pts, M, fmad=1)
        with _fmad(F):
            got = F.farthest_point_sample(_t(pts, dev), M).cpu().numpy()
            assert np.array_equal(got, want), (kind, form, _first_diff(got, want))
            _check_form(F, oracle, pts, M, dev, form, want, fmad=True, what=kind)


@pytest.mark.parametrize("contract", ["strict", "fmad"])
@pytest.mark.parametrize("N,M,mode", DE.FPS_PICK_DISTANCES)
def test_fps_pick_distances_feed_the_prefix_proof(F, oracle, dev, monkeypatch, N, M, mode, contract):
    """reg, pruned and pruned-L2 at both ends of their ranges: idx is the oracle's, ctr the gathered coordinates and
    dist[k] the running minimum pick k had, all bit for bit in the contract in force; s4g_fps_prefix_check_f32 then
    proves the tie-free cloud a prefix (run flag 0) and sends the lattice cloud to the sampler (run flag 1)."""
    _set_fps_mode(monkeypatch, mode)
    fmad = contract == "fmad"
    form = {(n, m, md): f for n, m, md, f in DE.fps_cases()}[(N, M, mode)]
    clouds = DE.fps_inputs(N, M)
    M2 = DE.prefix_steps(M)
    for kind, flag in (("uniform", 0), ("lattice", 1)):
        pts = clouds[kind]
        want = oracle.fps(pts, M, fmad=int(fmad))
        with _fmad(F, fmad):
            ctr, dist = _check_form(F, oracle, pts, M, dev, form, want, fmad=fmad, what=kind)
            run = _prefix_check(ctr, dist, M2, dev).cpu().tolist()
        assert run == [flag, flag], (kind, run)
        for b in range(2):
            assert DE.prefix_is_proven(ctr[b], dist[b], M2, fmad) == (flag == 0), (kind, b)
        if flag == 0:
            assert np.array_equal(oracle.fps(ctr, M2, fmad=int(fmad)), np.tile(np.arange(M2), (2, 1)))


@pytest.mark.parametrize("N,M,mode,full,null,short", DE.FPS_WORKSPACE)
def test_fps_workspace_fallback(F, oracle, dev, monkeypatch, N, M, mode, full, null, short):
    """With the workspace the library asks for, with none, and with one byte too few: the same indices each time, or
    S4G_EWORKSPACE where the streaming kernel has no buffer -- and then nothing is written."""
    from s4g_release_amd import _cabi
    _set_fps_mode(monkeypatch, mode)
    for kind, pts in DE.fps_inputs(N, M).items():
        want = oracle.fps(pts, M)
        for ws_kind, outcome in (("full", full), ("null", null), ("short", short)):
            rc, idx, ctr, _, touched = _fps_call(F, pts, M, dev, want_dist=False, ws_kind=ws_kind)
            if outcome == "EWORKSPACE":
                assert rc == _cabi.S4G_EWORKSPACE, (kind, ws_kind, rc)
                assert (idx == -7).all() and (ctr == -7.0).all() and not touched, (kind, ws_kind)
                continue
            assert rc == 0, (kind, ws_kind, rc)
            assert np.array_equal(idx, want), (kind, ws_kind, _first_diff(idx, want))
            assert np.array_equal(_bits(ctr), _bits(oracle.gather_points(pts, want))), (kind, ws_kind)
            base = outcome.split("<")[0]
            if ws_kind != "null":
                assert touched == (base != "reg"), (kind, ws_kind, outcome)
            # the form that answered, by whether it can report pick distances
            rc, idx, _, _, _ = _fps_call(F, pts, M, dev, want_dist=True, ws_kind=ws_kind)
            assert rc == (_cabi.S4G_EUNSUPPORTED if base == "stream" else 0), (kind, ws_kind, outcome, rc)
            assert (idx == -7).all() if base == "stream" else np.array_equal(idx, want), (kind, ws_kind)


# ------------------------------------------------------------------------------------------------------ ball query
@pytest.mark.parametrize("N,K,mode,path", DE.bq_cases())
def test_ball_query_ladder(F, oracle, dev, monkeypatch, N, K, mode, path):
    """Both sides of N = 8 192 (auto), of GR_MAX_POINTS and of K = 1 024, under auto and under the forced grid where
    it is legal: index and count against the oracle on a scene with empty, short and full balls; the workspace size
    says which path answers."""
    from s4g_release_amd import _cabi
    monkeypatch.setenv("S4G_BQ_MODE", mode)
    pts, ctr, r = DE.bq_inputs(N, K)
    ridx, rcnt = oracle.ball_query(pts, ctr, r, K)
    assert DE.bq_has_all_ball_kinds(rcnt, K)
    nbytes = _cabi.lib().s4g_workspace_bytes(_cabi.S4G_OP_BALL_QUERY, 2, N, DE.BQ_M, K)
    assert (nbytes != 0) == (path == "grid"), nbytes
    idx, cnt = F.ball_query(_t(pts, dev), _t(ctr, dev), r, K)
    assert idx.dtype == torch.int64 and cnt.dtype == torch.int64
    assert np.array_equal(cnt.cpu().numpy(), rcnt)
    assert np.array_equal(idx.cpu().numpy(), ridx)
    if K == 64:       # the fused operator on both paths of every size
        i2, c2, g2 = F.query_and_group(_t(pts, dev), _t(ctr, dev), r, K)
        assert torch.equal(i2, idx) and torch.equal(c2, cnt)
        assert np.array_equal(_bits(g2.cpu().numpy()), _bits(oracle.group_points(pts, ridx)))


def test_query_group_equals_the_operator_pair_on_the_scan_path(F, oracle, dev, monkeypatch):
    """One below the grid's first size: s4g_query_group_f32 = s4g_ball_query_f32 then s4g_group_points_f32."""
    monkeypatch.setenv("S4G_BQ_MODE", "auto")
    N, K = DE.BQ_GRID_MIN_N - 1, 64
    pts, ctr, r = DE.bq_inputs(N, K)
    idx, cnt = F.ball_query(_t(pts, dev), _t(ctr, dev), r, K)
    grouped = F.group_points(_t(pts, dev), idx)
    i2, c2, g2 = F.query_and_group(_t(pts, dev), _t(ctr, dev), r, K)
    assert torch.equal(i2, idx) and torch.equal(c2, cnt) and torch.equal(g2, grouped)
    ridx, rcnt = oracle.ball_query(pts, ctr, r, K)
    assert np.array_equal(i2.cpu().numpy(), ridx) and np.array_equal(c2.cpu().numpy(), rcnt)


# ------------------------------------------------------------------------------------------------------------ 3-NN
@pytest.mark.parametrize("N2,knob,value,path", DE.nn_cases())
def test_three_nn_ladder(F, oracle, dev, monkeypatch, N2, knob, value, path):
    """The operator API at every routing threshold (the minimum of three keys, the split scan's range, its 4 / 8 lane
    forms with a remainder of one key, the grid's range) and on the other side of the knob that decides there:
    indices and squared distances bit for bit, strict and fmad, tie-free and tie-heavy."""
    for name in ("S4G_NN_MODE", "S4G_NN_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    if knob:
        monkeypatch.setenv(knob, value)
    for kind, (q, k) in DE.nn_inputs(N2).items():
        for fmad in (False, True):
            ridx, rd2 = oracle.three_nn(q, k, fmad=int(fmad))
            with _fmad(F, fmad):
                idx, d2 = F.search_nn_distance(_t(q, dev), _t(k, dev), 3)
                i32, w = F.three_nn_weights(_t(q, dev), _t(k, dev))
            assert idx.dtype == torch.int64
            assert np.array_equal(idx.cpu().numpy(), ridx), (kind, fmad, path)
            assert np.array_equal(_bits(d2.cpu().numpy()), _bits(rd2)), (kind, fmad, path)
            assert np.array_equal(i32.cpu().numpy().astype(np.int64), ridx), (kind, fmad)
            assert np.array_equal(_bits(w.cpu().numpy()), _bits(oracle.interp_weights(rd2))), (kind, fmad)


@pytest.mark.parametrize("cell", [-1.0, 0.05])
@pytest.mark.parametrize("N2", DE.NN_GRID_ENTRY_N2)
def test_three_nn_grid_entry_ladder(F, oracle, dev, N2, cell):
    """s4g_three_nn_weights_grid_i32 called directly from three keys to GR_MAX_POINTS, with a named cell edge and with
    the edge chosen on the device: the scan's indices and weights whatever the cell."""
    for kind, (q, k) in DE.nn_inputs(N2).items():
        ridx, rd2 = oracle.three_nn(q, k)
        idx, w = F.three_nn_weights_grid(_t(q, dev), _t(k, dev), cell)
        assert idx.dtype == torch.int32
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), ridx), kind
        assert np.array_equal(_bits(w.cpu().numpy()), _bits(oracle.interp_weights(rd2))), kind


@pytest.mark.parametrize("cell", [-1.0, 0.05])
def test_three_nn_grid_entry_refuses_more_than_gr_max_points(F, dev, cell):
    """One key past GR_MAX_POINTS: S4G_EINVAL (bad size), nothing launched, nothing written."""
    from s4g_release_amd import _cabi
    N2, N1 = DE.NN_GRID_MAX + 1, DE.NN_N1
    q, k = DE.nn_inputs(N2)["tabletop"]
    qd, kd = _t(q, dev), _t(k, dev)
    idx = torch.full((2, N1, 3), -7, dtype=torch.int32, device=dev)
    w = torch.full((2, N1, 3), -7.0, dtype=torch.float32, device=dev)
    nbytes = _cabi.lib().s4g_three_nn_grid_workspace_bytes(2, N1, N2)
    ws = torch.full((nbytes,), MARK, dtype=torch.uint8, device=dev)
    rc = _cabi.lib().s4g_three_nn_weights_grid_i32(qd.data_ptr(), kd.data_ptr(), 2, N1, N2, 1e-10, cell,
                                                   idx.data_ptr(), w.data_ptr(), ws.data_ptr(), nbytes, F._DIST_FLAGS,
                                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _cabi.S4G_EINVAL
    assert (idx == -7).all() and (w == -7.0).all() and (ws == MARK).all()
    with pytest.raises(RuntimeError):
        F.three_nn_weights_grid(qd, kd, cell)
    # the operator API routes this size to the scan instead
    i64, _ = F.search_nn_distance(qd, kd, 3)
    assert i64.shape == (2, N1, 3) and int(i64.max()) < N2 and int(i64.min()) >= 0
