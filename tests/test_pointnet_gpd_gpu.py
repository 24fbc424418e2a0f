"""The PointNetGPD classifier on the device (`baselines.FusedPointNetGPD`, `postprocess.score_close_regions`;
csrc/pointnet_gpd.hip) against the float64 yardstick of tests/pointnet_gpd_ref.py (held to the reference's own network by
tests/test_pointnet_gpd_ref.py).

Parity bound per level: max(1e-4, 3 x margin[level]) of the tensor's scale.  1e-4 is the project's model-level bound;
the 3 x over the reference's own fp32 distance from float64 allows for the f16x2 split's fp32-dot-product error in
another summation order (measured at 0.7 - 3.2 x torch-CPU-fp32's distance on calibrated statistics, README round 4).
Measured on an MI355X: see PARITY_MEASURED below.  The exact constructions turn every stage into sums, maxima and
selections of small integers / 8, which the f16x2 split carries without rounding: bit for bit.

The C ABI calls put every output and the workspace inside sentinel-filled buffers with guard words on both sides."""
import ctypes

import numpy as np
import pytest
import torch

from tests import pointnet_gpd_ref as PR

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -559038737
TOL = 1e-4
T = 128                 # rows per tile of the trunk kernel (csrc/pointnet_gpd.hip)
R = 32                  # sets per workgroup of the per-set layers (csrc/pointnet_gpd.hip)
LEVELS = PR.LEVELS
SHAPES = {"stn_global": (1024,), "trans": (3, 3), "global": (1024,), "hidden": (256,)}


def _runner(state, dev, eps=None):
    from s4g_release_amd.baselines import FusedPointNetGPD, PointNetGPDClassifier
    net = PointNetGPDClassifier(3, state["fc3.weight"].shape[0])
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()}, strict=True)
    if eps is not None:
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.eps = eps
    return FusedPointNetGPD(net.to(dev).eval())


_CACHE = {}


def _net(dev):
    """(state, runner) of the fixture's calibrated network, built once."""
    if "net" not in _CACHE:
        state = PR.fixture_state(PR.load_fixture())
        _CACHE["net"] = (state, _runner(state, dev))
    return _CACHE["net"]


def _small_sets():
    """40 sets of 1 .. 40 points (`hashed_subset` of the real sets) and their float64 levels, built once."""
    if "small" not in _CACHE:
        real = PR.real_sets()
        sets = [PR.hashed_subset(real[i % 26], 1 + (7 * i) % 40, 50 + i) for i in range(40)]
        _CACHE["small"] = (sets, PR.forward64(PR.fixture_state(PR.load_fixture()), sets))
    return _CACHE["small"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _pack(sets, slack=5, fill=7.0e8):
    """One scene: points (1, 3, capacity), offset (1, F + 1), count (1, F); the slack behind the last set holds a huge
    finite value that no set may read."""
    count = np.asarray([s.shape[1] for s in sets], np.int32)
    offset = np.concatenate([[0], np.cumsum(count, dtype=np.int64)])
    pts = np.full((1, 3, int(offset[-1]) + slack), fill, np.float32)
    for s, o in zip(sets, offset):
        pts[0, :, o:o + s.shape[1]] = s
    return pts, offset[None].astype(np.int64), count[None]


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _forward_guarded(dev, run, points, G, offset=None, count=None, flags=None, index=None, chunk=0, expect=0):
    """s4g_pngpd_forward_f32 through the C ABI, every output and the workspace guarded.  points: numpy (n, 3, npts)
    (dense) or (B, 3, capacity) with offset / count (packed) -> dict level -> numpy array, "status" included."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    lib = _cabi.lib()
    K = run.classes
    packed = run.pack(dev)
    shapes = {"logits": (G, K), "status": (G,)}
    shapes.update({k: (G,) + s for k, s in SHAPES.items()})
    bufs = {k: _guarded(s, dev) for k, s in shapes.items()}
    nbytes = int(lib.s4g_pngpd_workspace_bytes(min(chunk, G) if chunk else min(1024, max(G, 1)), K))
    ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)   # noqa: E731
    d_pts, d_off, d_cnt = t(points, np.float32), t(offset, np.int64), t(count, np.int32)
    d_flg, d_idx = t(flags, np.int32), t(index, np.int32)
    ptr = lambda a: None if a is None else a.data_ptr()   # noqa: E731
    B, _, cap = points.shape
    if offset is None:
        args = (3 * cap, cap, cap, None, None, None, 0, 0, ptr(d_idx), G, B)
    else:
        Fr = count.shape[1]
        args = (3 * cap, cap, 0, ptr(d_off), ptr(d_cnt), ptr(d_flg), Fr, cap, ptr(d_idx), G, B * Fr)
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    with torch.cuda.device(dev):
        rc = lib.s4g_pngpd_forward_f32(d_pts.data_ptr(), *args, packed.data_ptr(), K, chunk, p["stn_global"], p["trans"],
                                       p["global"], p["hidden"], p["status"], p["logits"], ws[GUARD * 4:].data_ptr(),
                                       nbytes, Fn._stream())
    assert rc == expect, rc
    torch.cuda.synchronize(dev)
    for k, (buf, _) in bufs.items():
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "guard of %s" % k
    assert (ws[:GUARD * 4] == 0x5A).all() and (ws[GUARD * 4 + nbytes:] == 0x5A).all(), "guard of the workspace"
    out = {k: v.cpu().numpy().reshape(shapes[k]) for k, (_, v) in bufs.items()}
    return {k: (v if k == "status" else v.view(np.float32)) for k, v in out.items()}


def _packed_guarded(dev, run, sets, **kw):
    pts, off, cnt = _pack(sets)
    G = len(kw["index"]) if kw.get("index") is not None else len(sets)
    return _forward_guarded(dev, run, pts, G, offset=off, count=cnt, **kw)


def _distances(got, want, rows=None):
    return {k: PR.distance(got[k], want[k] if rows is None else want[k][rows]) for k in LEVELS}


def _check64(got, want, rows=None, what="", bound=None):
    d = _distances(got, want, rows)
    for k in LEVELS:
        assert np.isfinite(got[k]).all() and d[k] <= (TOL if bound is None else bound[k]), (what, k, d[k])
    return d


def _same_rows(a, ra, b, rb):
    return all(np.array_equal(_bits(a[k][ra]), _bits(b[k][rb])) for k in LEVELS)


def _call(run, points, **kw):
    logits, f = run(points, features=True, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in f.items()}
    out["logits"] = logits.cpu().numpy()
    return out


# ------------------------------------------------------------------------------------------------------------- parity
# max |device - float64| / scale on an MI355X, (stn_global, trans, global, hidden, logits); see the profile
PARITY_MEASURED = (4.1e-7, 1.3e-6, 3.9e-6, 3.3e-6, 2.3e-6)     # packed and dense alike (the same bits)


def test_parity_with_the_fixture(dev):
    fx = PR.load_fixture()
    state, run = _net(dev)
    sets = PR.fixture_sets()
    want = PR.forward64(state, sets)
    bound = {k: max(TOL, 3.0 * float(fx["margin/" + k][0])) for k in LEVELS}
    packed = _packed_guarded(dev, run, sets, chunk=8)
    assert not packed["status"].any()
    d = _check64(packed, want, what="packed", bound=bound)
    print("pointnet_gpd parity (packed):", {k: "%.3g" % v for k, v in d.items()})
    dense = {k: [] for k in LEVELS}
    for s in sets:                                                  # the dense form holds sets of one size: one call each
        got = _forward_guarded(dev, run, s[None], 1)
        for k in LEVELS:
            dense[k].append(got[k][0])
    dense = {k: np.stack(v) for k, v in dense.items()}
    d = _check64(dense, want, what="dense", bound=bound)
    print("pointnet_gpd parity (dense):", {k: "%.3g" % v for k, v in d.items()})
    assert _same_rows(dense, slice(None), packed, slice(None))
    for got in (packed, dense):
        for k in LEVELS:
            assert PR.distance(got[k], fx[k].astype(np.float64)) <= bound[k], k


# ------------------------------------------------------------------------------------------------ exact constructions
TRANS = np.asarray([[1, 1, 0], [-1, 1, 0], [0, 2, 2]], np.float64)


def _integer_state(classes):
    """One-hot and small-integer weights, integer biases, identity BatchNorm (gamma 1, beta 0, mean 0, var 1; the runner
    is built with eps 0), feat.stn.fc3 = 0 with the integer bias TRANS - I.  feat.conv3's biases lie at -24 .. -20, so a
    set of small coordinates has only negative feature maxima."""
    st = {k: np.zeros_like(v) for k, v in PR.hashed_state(classes).items()}
    for k in st:
        if k.endswith("running_var") or (k.endswith("weight") and ".bn" in "." + k):
            st[k] = np.ones_like(st[k])
    def fill(name, second, bias):       # noqa: E306
        w = st[name + ".weight"].reshape(st[name + ".weight"].shape[0], -1)
        out, cin = w.shape
        for o in range(out):
            w[o, (o * 5) % cin] = 1 + o % 2
            if second:
                w[o, (o * 7 + 3) % cin] += -1 if o % 3 else 1
        st[name + ".bias"][:] = bias(np.arange(out))
    fill("feat.stn.conv1", True, lambda o: o % 3 - 1)
    fill("feat.stn.conv2", True, lambda o: o % 4 - 2)
    fill("feat.stn.conv3", True, lambda o: o % 5 - 3)
    fill("feat.stn.fc1", False, lambda o: o % 3 - 1)
    fill("feat.stn.fc2", False, lambda o: o % 2)
    st["feat.stn.fc3.bias"][:] = (TRANS - np.eye(3)).reshape(9)
    fill("feat.conv1", True, lambda o: o % 3 - 1)
    fill("feat.conv2", True, lambda o: o % 4 - 2)
    fill("feat.conv3", True, lambda o: o % 5 - 24)
    fill("fc1", False, lambda o: 30 - o % 3)
    fill("fc2", False, lambda o: o % 4 - 1)
    units = [0, 31, 32, 127, 128, 255, 1, 2, 3, 4, 5, 6, 63, 64, 65, 200]
    for c in range(classes):
        st["fc3.weight"][c, units[c]] = 1 + c % 2
    st["fc3.bias"][:] = np.arange(classes) - 1
    return st


def _integer_sets():
    """Coordinates k / 8: sizes on both sides of the tile, one set of small coordinates (|x| <= 1 / 8)."""
    sizes = (1, 5, T - 1, T, T + 1, 2 * T + 1, 40)
    sets = [np.round(PR._unit(3 * n, 300 + i).reshape(3, n) * 12.0) / 8.0 for i, n in enumerate(sizes)]
    sets[-1] = np.round(sets[-1] / 1.5 * 8.0 / 12.0) / 8.0
    return [s.astype(np.float32) for s in sets]


@pytest.mark.parametrize("classes", (16, 3))
def test_exact_constructions(dev, classes):
    st, sets = _integer_state(classes), _integer_sets()
    want = PR.forward64(st, sets, eps=0.0)
    assert np.array_equal(want["trans"][0], TRANS)
    assert (want["global"][-1] < 0).all() and (want["global"][2] > 0).any() and (want["global"][2] < 0).any()
    assert want["hidden"].max() > 0 and np.ptp(want["logits"]) > 0 and np.ptp(want["stn_global"]) > 0
    run = _runner(st, dev, eps=0.0)
    order = [3, 0, 6, 5, 1, 2, 4]
    got = _packed_guarded(dev, run, sets, index=order, chunk=3)
    for k in LEVELS:
        assert np.array_equal(_bits(got[k]), _bits(want[k][order].astype(np.float32))), k
    for i in (1, 6):                                                 # and dense
        one = _forward_guarded(dev, run, sets[i][None], 1)
        assert _same_rows(one, 0, got, order.index(i))


# ------------------------------------------------------------------------------------------------------ set-size edges
def test_set_size_edges(dev):
    state, run = _net(dev)
    real = PR.real_sets()
    sizes = (2 * T, 1, T + 1, 2, T - 1, 2 * T + 1, T)
    sets = [PR.hashed_subset(real[2 * i], n, 70 + i) for i, n in enumerate(sizes)]
    want = PR.forward64(state, sets)
    got = _packed_guarded(dev, run, sets)
    _check64(got, want, what="sizes")
    for i in range(len(sets)):
        _check64({k: got[k][i:i + 1] for k in LEVELS}, {k: want[k][i:i + 1] for k in LEVELS}, what=("size", sizes[i]))
        assert _same_rows(_packed_guarded(dev, run, [sets[i]]), 0, got, i), sizes[i]


def test_decisive_point_positions(dev):
    """On the integer network (bit for bit): the one point that decides feature channel 0 sits first, last, on the last
    row of a full tile, and alone in a one-row last tile."""
    st = _integer_state(3)
    run = _runner(st, dev, eps=0.0)
    cases = ((T, 0), (T, T - 1), (2 * T, T - 1), (T + 1, T), (2 * T + 1, 2 * T), (2 * T + 1, 0))
    sets, without = [], []
    for i, (n, p) in enumerate(cases):
        s = (np.round(PR._unit(3 * n, 400 + i).reshape(3, n) * 2.0) / 8.0).astype(np.float32)
        s[:, p] = (1.5, -0.75, 2.0)
        sets.append(s)
        without.append(np.delete(s, p, axis=1))
    want, lack = PR.forward64(st, sets, eps=0.0), PR.forward64(st, without, eps=0.0)
    ch = int(np.argmax((want["global"] > lack["global"]).all(axis=0)))
    assert (want["global"][:, ch] > lack["global"][:, ch]).all(), "no channel is decided by the placed point in every set"
    got = _packed_guarded(dev, run, sets)
    for k in LEVELS:
        assert np.array_equal(_bits(got[k]), _bits(want[k].astype(np.float32))), k


def test_neighbours_of_very_different_scale(dev):
    state, run = _net(dev)
    real = PR.real_sets()
    a = (real[4][:, :150] * np.float32(1e4)).astype(np.float32)       # coordinates around 1e3
    b = (real[5][:, :150] * np.float32(1e-2)).astype(np.float32)      # around 1e-3
    assert 100 < np.abs(a).max() < 2e3 and 1e-4 < np.abs(b).max() < 2e-3
    alone = [_packed_guarded(dev, run, [s]) for s in (a, b)]
    for sets, rows in (((a, b), (0, 1)), ((b, a), (1, 0)), ((b, a, b), (1, 0, 1))):
        got = _packed_guarded(dev, run, list(sets))
        for g, r in enumerate(rows):
            assert _same_rows(got, g, alone[r], 0), (len(sets), g)
    _check64(alone[1], PR.forward64(state, [b]), what="1e-3")
    _check64(alone[0], PR.forward64(state, [a]), what="1e3")


# ----------------------------------------------------------------------------------------------------- set-count edges
@pytest.mark.parametrize("G", (1, R - 1, R, R + 1))
def test_set_count_and_chunk_edges(dev, G):
    state, run = _net(dev)
    sets, want = _small_sets()
    base = _packed_guarded(dev, run, sets[:G])
    _check64(base, want, slice(0, G), ("G", G))
    for chunk in sorted({1, R, G - 1, G} - {0}):
        got = _packed_guarded(dev, run, sets[:G], chunk=chunk)
        assert _same_rows(got, slice(None), base, slice(None)), (G, chunk)


# -------------------------------------------------------------------------------------------------------------- states
def test_states(dev):
    state, run = _net(dev)
    sets, want = _small_sets()
    sets = sets[:8]
    pts, off, cnt = _pack(sets)
    plain = _forward_guarded(dev, run, pts, 8, offset=off, count=cnt)
    _check64(plain, want, slice(0, 8))
    # an empty set, a flagged set, index -1, index >= F, a repeated index
    cnt2, off2 = cnt.copy(), off.copy()
    cnt2[0, 3] = 0
    flags = np.zeros((1, 8), np.int32)
    flags[0, 5] = 1
    flags[0, 6] = 2                                                  # bit 1 alone does not stop the scoring
    index = [0, 3, 5, -1, 8, 100, 6, 2, 2, 7]
    got = _forward_guarded(dev, run, pts, len(index), offset=off2, count=cnt2, flags=flags, index=index, chunk=4)
    assert list(got["status"]) == [0, 2, 2, 2, 2, 2, 0, 0, 0, 0]
    for g, src in enumerate(index):
        if got["status"][g] == 2:
            assert all(not _bits(got[k][g]).any() for k in LEVELS), g
        else:
            assert _same_rows(got, g, plain, src), g
    assert _same_rows(got, 7, got, 8)
    # a slice that leaves the buffer is not read
    cnt3 = cnt.copy()
    cnt3[0, 7] = pts.shape[2]
    got = _forward_guarded(dev, run, pts, 8, offset=off, count=cnt3)
    assert got["status"][7] == 2 and not got["status"][:7].any() and _same_rows(got, slice(0, 7), plain, slice(0, 7))
    # one NaN, one infinity
    for bad, (s, c, j) in ((np.nan, (2, 1, 0)), (np.inf, (4, 2, -1)), (-np.inf, (7, 0, 3))):
        hurt = pts.copy()
        hurt[0, c, off[0, s] + (j % cnt[0, s])] = bad
        got = _forward_guarded(dev, run, hurt, 8, offset=off, count=cnt, chunk=3)
        assert list(got["status"]) == [int(i == s) for i in range(8)]
        assert all(np.isnan(got[k][s]).all() for k in LEVELS)
        keep = [i for i in range(8) if i != s]
        assert _same_rows(got, keep, plain, keep)


# ----------------------------------------------------------------------------------------------------------- invariance
def test_invariance_and_graph_replay(dev):
    state, run = _net(dev)
    real = PR.real_sets()
    n = 200
    sets = [PR.hashed_subset(real[3 * i], n, 90 + i) for i in range(6)]
    dense = np.stack(sets)                                            # (6, 3, 200)
    want = PR.forward64(state, sets)
    d_dense = torch.from_numpy(dense).to(dev)
    got_dense = _call(run, d_dense)
    _check64(got_dense, want)
    assert not got_dense["status"].any()
    pts, off, cnt = _pack(sets)
    d = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    d_pts, d_off, d_cnt = d(pts), d(off), d(cnt)
    got_packed = _call(run, d_pts, offset=d_off, count=d_cnt)
    assert got_packed["logits"].shape == (1, 6, 3) and got_packed["trans"].shape == (1, 6, 3, 3)
    flat = {k: v.reshape((6,) + v.shape[2:]) for k, v in got_packed.items()}
    assert _same_rows(flat, slice(None), got_dense, slice(None))
    four = _call(run, d_dense.reshape(2, 3, 3, n))                    # (B, K, 3, n)
    assert four["logits"].shape == (2, 3, 3)
    assert _same_rows({k: v.reshape((6,) + v.shape[2:]) for k, v in four.items()}, slice(None), got_dense, slice(None))
    for i in (0, 3, 5):                                               # alone, and at any position, for any chunk
        alone = _call(run, d_dense[i:i + 1])
        assert _same_rows(alone, 0, got_dense, i)
        for pos in (0, 2, 5):
            order = list(range(6))
            order[pos], order[i] = order[i], order[pos]
            for chunk in (None, 1, 4):
                moved = _call(run, d_dense[order], chunk=chunk)
                assert _same_rows(moved, pos, alone, 0), (i, pos, chunk)
    again = _call(run, d_dense)
    assert _same_rows(again, slice(None), got_dense, slice(None))
    # (B, K) index within the scene, -1 = a zero row
    idx = torch.tensor([[5, -1, 0, 0]], device=dev)
    sel = _call(run, d_pts, offset=d_off, count=d_cnt, index=idx)
    assert sel["logits"].shape == (1, 4, 3) and list(sel["status"][0]) == [0, 2, 0, 0]
    for j, r in enumerate((5, None, 0, 0)):
        for k in LEVELS:
            g = sel[k][0, j]
            assert np.array_equal(_bits(g), _bits(got_dense[k][r]) if r is not None else np.zeros_like(_bits(g))), (j, k)
    # one capture and one replay on the single current stream
    buf = d_pts.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        logits, f = run(buf, offset=d_off, count=d_cnt, features=True, chunk=4)
    outs = dict(f, logits=logits)
    for v in outs.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    rep = {k: v.cpu().numpy().reshape((6,) + tuple(v.shape[2:])) for k, v in outs.items()}
    assert _same_rows(rep, slice(None), got_dense, slice(None)) and not rep["status"].any()


# ----------------------------------------------------------------------------------------------------------- end to end
def test_score_close_regions_end_to_end(dev):
    from s4g_release_amd import postprocess as PP
    from tests import close_region_ref as CR
    fx = CR.load_fixture()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    labels = PP.label_baseline_view(t(fx["points"]), t(fx["frames"]), t(fx["cloud"]), t(fx["normals"]))
    state, run = _net(dev)
    run.pack(dev)
    torch.cuda.synchronize(dev)
    r = labels.regions
    count = int(labels.best.count[0])
    Fr = r.count.shape[1]
    assert count >= 20 and count < Fr
    vi = labels.best.valid_index[0].cpu().numpy()
    off, cnt, P = r.offset[0].cpu().numpy(), r.count[0].cpu().numpy(), r.points[0].cpu().numpy()
    sets = [P[:, off[f]:off[f] + cnt[f]] for f in vi[:count]]
    assert min(s.shape[1] for s in sets) >= 1 and not r.flags[0].cpu().numpy()[vi[:count]].any()
    # the runner on the corresponding sets, each alone in the dense form
    alone = np.stack([_call(run, t(s[None]))["logits"][0] for s in sets])
    want = PR.forward64(state, sets)["logits"]
    assert PR.distance(alone, want) <= TOL
    for grasp_num in (count - 3, count, count + 4, None):
        g = torch.cuda.CUDAGraph()                                    # a host sync inside would fail the capture
        with torch.cuda.graph(g):
            out = PP.score_close_regions(labels, run, grasp_num)
        g.replay()
        torch.cuda.synchronize(dev)
        K = Fr if grasp_num is None else min(grasp_num, Fr)
        assert tuple(out.shape) == (1, K, 3)
        got = out[0].cpu().numpy()
        n = min(K, count)
        assert np.array_equal(_bits(got[:n]), _bits(alone[:n]))
        assert not _bits(got[n:]).any()
    every = PP.score_close_regions(labels.regions, run)
    torch.cuda.synchronize(dev)
    assert tuple(every.shape) == (1, Fr, 3)
    assert np.array_equal(_bits(every[0].cpu().numpy()[vi[:count]]), _bits(alone))
    with pytest.raises(RuntimeError):
        PP.score_close_regions(labels.regions, run, grasp_num=3)
    with pytest.raises(ValueError):
        PP.score_close_regions(labels, run, grasp_num=-1)


# ---------------------------------------------------------------------------------------------------------- host checks
def test_host_checks_on_the_device(dev):
    from s4g_release_amd import _cabi
    state, run = _net(dev)
    ok = torch.zeros(2, 3, 50, device=dev)
    for bad in (ok.double(), ok.half(), ok[0, 0], ok[:, :2], torch.zeros(2, 4, 50, device=dev)):
        with pytest.raises(RuntimeError):
            run(bad)
    off, cnt = torch.zeros((2, 3), dtype=torch.int64, device=dev), torch.zeros((2, 2), dtype=torch.int32, device=dev)
    for kw in (dict(offset=off), dict(count=cnt), dict(offset=off[:, :2], count=cnt), dict(offset=off.int(), count=cnt),
               dict(offset=off, count=cnt.long()), dict(offset=off, count=cnt, flags=cnt[:, :1]),
               dict(offset=off, count=cnt, index=torch.zeros((3, 1), dtype=torch.int64, device=dev)),
               dict(offset=off, count=cnt, index=torch.zeros(2)), dict(index=torch.zeros(2, dtype=torch.int64, device=dev))):
        with pytest.raises(RuntimeError):
            run(ok, **kw)
    with pytest.raises(ValueError):
        run(ok, chunk=0)
    run.net.train()
    run._packed = None
    with pytest.raises(RuntimeError, match="eval"):
        run(ok)
    run.net.eval()
    assert tuple(run(ok[:0]).shape) == (0, 3)
    out, f = run(ok, offset=off, count=cnt, features=True)            # every set is empty: zero rows, status 2
    torch.cuda.synchronize(dev)
    assert tuple(out.shape) == (2, 2, 3) and not out.any() and (f["status"] == 2).all()
    lib = _cabi.lib()
    assert lib.s4g_pngpd_pack_bytes(17) == 0 and lib.s4g_pngpd_pack_bytes(0) == 0 and lib.s4g_pngpd_pack_bytes(3) > 0
    assert lib.s4g_pngpd_workspace_bytes(3, 3) < lib.s4g_pngpd_workspace_bytes(4, 3)
    assert lib.s4g_pngpd_workspace_bytes(0, 3) == lib.s4g_pngpd_workspace_bytes(1024, 3)
    assert lib.s4g_pngpd_workspace_bytes(32769, 3) == 0
    sets, _ = _small_sets()
    pts, o, c = _pack(sets[:4])
    _forward_guarded(dev, run, pts, 5, offset=o, count=c, expect=_cabi.S4G_EINVAL)      # G > num_sets without an index
    packed, logits = run.pack(dev), torch.zeros(2, 3, device=dev)
    ws = torch.zeros(int(lib.s4g_pngpd_workspace_bytes(2, 3)), dtype=torch.uint8, device=dev)
    args = lambda K=3, chunk=0, nb=ws.numel(), npts=50: (ok.data_ptr(), 150, 50, npts, None, None, None, 0, 0, None, 2, 2,  # noqa: E731
                                                        packed.data_ptr(), K, chunk, None, None, None, None, None,
                                                        logits.data_ptr(), ws.data_ptr(), nb, None)
    assert lib.s4g_pngpd_forward_f32(*args(K=17)) == _cabi.S4G_EINVAL
    assert lib.s4g_pngpd_forward_f32(*args(chunk=-1)) == _cabi.S4G_EINVAL
    assert lib.s4g_pngpd_forward_f32(*args(npts=-1)) == _cabi.S4G_EINVAL
    assert lib.s4g_pngpd_forward_f32(*args(nb=ws.numel() - 1)) == _cabi.S4G_EWORKSPACE
    null12 = (ctypes.c_void_p * 12)()
    assert lib.s4g_pngpd_pack_f32(ctypes.cast(null12, ctypes.c_void_p), ctypes.cast(null12, ctypes.c_void_p), 3,
                                  packed.data_ptr(), None) == _cabi.S4G_EINVAL
