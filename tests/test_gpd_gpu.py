"""The GPD classifier on the device (`baselines.FusedGPD`, `postprocess.score_projections`; csrc/gpd.hip) against the
float64 yardstick of tests/gpd_ref.py (held to the reference's own network by tests/test_gpd_ref.py).

Parity bound: 1e-4 of each tensor's scale at every level, the project's model-level bound.  Measured on an MI355X
(profiles/r16_gpd_classifier.md): see PARITY_MEASURED below.  The exact constructions turn every stage into sums, shifts,
maxima and selections of small integers, which the f16x2 split carries without rounding: bit for bit.

The edge tests call the C ABI with every output inside a sentinel-filled buffer with guard words on both sides, the
workspace included."""
import numpy as np
import pytest
import torch

from tests import gpd_ref as GR

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -559038737
TOL = 1e-4
LEVELS = ("pool1", "pool2", "hidden", "logits")
SHAPES = {"pool1": (20, 28, 28), "pool2": (50, 12, 12), "hidden": (500,)}
FC_ROWS = 32            # images per workgroup of the fc1 kernel (csrc/gpd.hip)


def _runner(state, dev):
    from s4g_release_amd.baselines import FusedGPD, GPDClassifier
    cin, classes = state["conv1.weight"].shape[1], state["fc2.weight"].shape[0]
    net = GPDClassifier(cin, classes)
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in state.items()},
                        strict=True)
    return FusedGPD(net.to(dev).eval())


_CACHE = {}


def _case(cin, classes, dev):
    """(state, runner, 7 images: 3 real maps, 3 dense, one zero, their float64 levels), built once per network."""
    key = (cin, classes)
    if key not in _CACHE:
        state = GR.hashed_state(cin, classes)
        full = GR.fixture_images(cin)
        images = np.ascontiguousarray(full[[0, 7, 19, 26, 27, 28, 32]])
        _CACHE[key] = (state, _runner(state, dev), images, GR.forward64(state, images))
    return _CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _forward_guarded(dev, run, maps, G, index=None, chunk=0, num_images=None, expect=0):
    """s4g_gpd_forward_f32 through the C ABI on maps (n, C, 60, 60) (a torch view; its strides are passed on), every
    output and the workspace guarded -> dict level -> fp32 numpy array."""
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    lib = _cabi.lib()
    cin, K = run.in_channels, run.classes
    packed = run.pack(dev)
    shapes = {"logits": (G, K)}
    shapes.update({k: (G,) + s for k, s in SHAPES.items()})
    bufs = {k: _guarded(s, dev) for k, s in shapes.items()}
    nbytes = int(lib.s4g_gpd_workspace_bytes(min(chunk, G) if chunk else min(1024, max(G, 1)), cin, K))
    ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
    d_idx = None if index is None else torch.as_tensor(np.asarray(index, np.int32), device=dev)
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    with torch.cuda.device(dev):
        rc = lib.s4g_gpd_forward_f32(maps.data_ptr(), maps.stride(0), maps.stride(1),
                                     None if d_idx is None else d_idx.data_ptr(), G,
                                     maps.shape[0] if num_images is None else num_images, packed.data_ptr(), cin, K, chunk,
                                     p["pool1"], p["pool2"], p["hidden"], p["logits"], ws[GUARD * 4:].data_ptr(), nbytes,
                                     Fn._stream())
    assert rc == expect, rc
    torch.cuda.synchronize(dev)
    for k, (buf, _) in bufs.items():
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "guard of %s" % k
    assert (ws[:GUARD * 4] == 0x5A).all() and (ws[GUARD * 4 + nbytes:] == 0x5A).all(), "guard of the workspace"
    return {k: v.cpu().numpy().view(np.float32).reshape(shapes[k]) for k, (_, v) in bufs.items()}


def _check64(got, want, rows=None, what=""):
    """Every level of `got` within TOL of scale of the yardstick rows `rows` -> the distances."""
    out = {}
    for k in LEVELS:
        w = want[k] if rows is None else want[k][rows]
        out[k] = GR.distance(got[k], w)
        assert np.isfinite(got[k]).all() and out[k] <= TOL, (what, k, out[k])
    return out


def _same_rows(a, ra, b, rb):
    return all(np.array_equal(_bits(a[k][ra]), _bits(b[k][rb])) for k in LEVELS)


def _call(run, maps, **kw):
    logits, f = run(maps, features=True, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in f.items()}
    out["logits"] = logits.cpu().numpy()
    return out


# ------------------------------------------------------------------------------------------------------------- parity
# max |device - float64| / scale on an MI355X, (pool1, pool2, hidden, logits); see the profile
PARITY_MEASURED = {12: (4.3e-7, 5.2e-7, 1.8e-6, 1.1e-6), 3: (3.7e-7, 4.8e-7, 1.7e-6, 1.4e-6)}


@pytest.mark.parametrize("cin,classes", ((12, 3), (3, 3)))
def test_parity_with_the_fixture_networks(dev, cin, classes):
    fx = GR.load_fixture()
    state, images = GR.hashed_state(cin, classes), GR.fixture_images(cin)
    want = GR.forward64(state, images)
    got = _call(_runner(state, dev), torch.from_numpy(images).to(dev))
    d = _check64(got, want, what="parity")
    print("gpd parity c%d:" % cin, {k: "%.3g" % v for k, v in d.items()})
    tag = "c%d" % cin
    sel = list(fx["level_images"])
    for k in LEVELS:
        g = got[k] if k in ("logits", "hidden") else got[k][sel]
        assert GR.distance(g, fx["%s/%s" % (tag, k)].astype(np.float64)) <= TOL + float(fx["%s/margin/%s" % (tag, k)][0])


# ------------------------------------------------------------------------------------------------ exact constructions
TAPS = ((0, 0), (0, 4), (4, 0), (4, 4), (2, 2))


def _integer_state(cin, classes):
    """One-hot conv kernels (weight 1 or 2) over the corners and centre of the window and the first, a middle and the
    last input channel, integer biases, one-hot fc rows."""
    st = {"conv1.weight": np.zeros((20, cin, 5, 5)), "conv1.bias": np.arange(20) % 3 - 1.0,
          "conv2.weight": np.zeros((50, 20, 5, 5)), "conv2.bias": np.arange(50) % 4 - 2.0,
          "fc1.weight": np.zeros((500, 7200)), "fc1.bias": (np.arange(500) % 5) * 6 - 20.0,
          "fc2.weight": np.zeros((classes, 500)), "fc2.bias": np.arange(classes) - 1.0}
    for name, chans in (("conv1.weight", sorted({0, cin // 2, cin - 1})), ("conv2.weight", [0, 10, 19])):
        w = st[name]
        for o in range(w.shape[0]):
            ky, kx = TAPS[o % 5]
            w[o, chans[(o // 5) % len(chans)], ky, kx] = 1 + o % 2
    # fc1 columns (c, y, x) -> c * 144 + y * 12 + x: the ends, both sides of the 8-element fragment and 16-wide k-step
    # boundaries, of conv2's strip boundary (pooled rows 5 | 6) in the first, a middle and the last channel, and of
    # its tile boundaries (pooled columns 3 | 4, 7 | 8)
    hot = [0, 7199, 7, 8, 15, 16, 7183, 7184, 7191, 7192]
    for c in (0, 25, 49):
        hot += [c * 144 + 5 * 12 + 11, c * 144 + 6 * 12, c * 144 + 5 * 12 + 3, c * 144 + 6 * 12 + 4,
                c * 144 + 7, c * 144 + 8]
    for u in range(500):
        st["fc1.weight"][u, hot[u % len(hot)] if u < 2 * len(hot) else (u * 37) % 7200] = 1 + u % 3
    # hidden units on both sides of the fc1 kernel's 128-unit workgroups and 32-unit tiles, and the last one
    units = [0, 31, 32, 127, 128, 255, 256, 383, 384, 499, 1, 2, 3, 4, 5, 6]
    for c in range(classes):
        st["fc2.weight"][c, units[c]] = 1.0
    return {k: v.astype(np.float32) for k, v in st.items()}


def _integer_forward(st, images):
    """The four levels in int64 arithmetic."""
    p = {k: v.astype(np.int64) for k, v in st.items()}
    x = images.astype(np.int64)
    p1 = GR._pool(GR._conv5(x, p["conv1.weight"]) + p["conv1.bias"][None, :, None, None])
    p2 = GR._pool(GR._conv5(p1, p["conv2.weight"]) + p["conv2.bias"][None, :, None, None])
    h = np.maximum(p2.reshape(len(x), 7200) @ p["fc1.weight"].T + p["fc1.bias"], 0)
    out = {"pool1": p1, "pool2": p2, "hidden": h, "logits": h @ p["fc2.weight"].T + p["fc2.bias"]}
    assert all(v.dtype == np.int64 for v in out.values())
    return out


@pytest.mark.parametrize("cin,classes", ((12, 16), (3, 3), (1, 1), (9, 2)))
def test_exact_constructions(dev, cin, classes):
    st = _integer_state(cin, classes)
    images = np.floor((GR._unit(5 * cin * 3600, 77 + cin) + 1.0) * 4.0).clip(0, 7).reshape(5, cin, 60, 60)
    images = images.astype(np.float32)
    assert images.max() == 7 and images.min() == 0
    want = _integer_forward(st, images)
    assert want["hidden"].max() > 0 and np.ptp(want["pool2"]) > 0
    got = _forward_guarded(dev, _runner(st, dev), torch.from_numpy(images).to(dev), 5, chunk=2)
    for k in LEVELS:
        assert np.array_equal(_bits(got[k]), _bits(want[k].astype(np.float32))), k


# ------------------------------------------------------------------------------------------------- edges against float64
@pytest.mark.parametrize("chunk,G", [(0, 1), (0, 2), (1, 1), (1, 2), (1, 3), (3, 2), (3, 3), (3, 4), (3, 7)])
def test_chunk_edges(dev, chunk, G):
    state, run, images, want = _case(3, 3, dev)
    got = _forward_guarded(dev, run, torch.from_numpy(images[:G]).to(dev), G, chunk=chunk)
    _check64(got, want, slice(0, G), (chunk, G))


@pytest.mark.parametrize("cin,classes", ((1, 1), (3, 3), (11, 16), (12, 3), (8, 2)))
def test_channel_and_class_counts(dev, cin, classes):
    state, run, images, want = _case(cin, classes, dev)
    got = _forward_guarded(dev, run, torch.from_numpy(images).to(dev), len(images), chunk=4)
    _check64(got, want, None, (cin, classes))


@pytest.mark.parametrize("G", (FC_ROWS - 1, FC_ROWS, FC_ROWS + 1))
def test_images_per_workgroup_edges(dev, G):
    """Rows of repeated images through `index`: each equals the unindexed row of its image, which the yardstick holds."""
    state, run, images, want = _case(12, 3, dev)
    d_maps = torch.from_numpy(images).to(dev)
    plain = _forward_guarded(dev, run, d_maps, len(images))
    _check64(plain, want)
    index = np.arange(G) % len(images)
    got = _forward_guarded(dev, run, d_maps, G, index=index)
    for g in range(G):
        assert _same_rows(got, g, plain, index[g]), g


def test_views_are_read_in_place(dev):
    """A 12-channel map read by a 3-channel network, a channel slice, and a (B, F) view with a frame stride."""
    state, run, images, want = _case(3, 3, dev)
    wide = np.concatenate([images, GR.hashed_images(len(images), 9, salt=5)], axis=1)          # (7, 12, 60, 60)
    d_wide = torch.from_numpy(wide).to(dev)
    plain = _call(run, torch.from_numpy(images).to(dev))
    _check64(plain, want)
    assert _same_rows(_call(run, d_wide), slice(None), plain, slice(None))
    shifted = torch.from_numpy(np.concatenate([wide[:, 9:], wide[:, :9]], axis=1)).to(dev)      # channels 3..5 = images
    view = shifted[:, 3:6]
    assert not view.is_contiguous()
    assert _same_rows(_call(run, view), slice(None), plain, slice(None))
    got = _forward_guarded(dev, run, view, len(images), chunk=3)
    assert _same_rows(got, slice(None), plain, slice(None))
    six = d_wide[:6].reshape(2, 3, 12, 60, 60)
    stepped = torch.stack([d_wide[[0, 6, 1, 6, 2, 6]], d_wide[[3, 6, 4, 6, 5, 6]]])[:, ::2]     # (2, 3, ...) strided
    assert stepped.stride(1) == 2 * 12 * 3600 and torch.equal(stepped, six)
    out = _call(run, stepped)
    assert out["logits"].shape == (2, 3, 3) and out["pool1"].shape == (2, 3, 20, 28, 28)
    for k in LEVELS:
        assert np.array_equal(_bits(out[k]).reshape((6,) + out[k].shape[2:]), _bits(plain[k][:6])), k
    # (B, K) rows index within their own scene
    idx = torch.tensor([[2, -1, 0, 0], [1, 2, 3, -1]], device=dev)
    out = _call(run, stepped, index=idx)
    rows = [2, None, 0, 0, 4, 5, None, None]
    for j, r in enumerate(rows):
        for k in LEVELS:
            g = out[k].reshape((8,) + out[k].shape[2:])[j]
            assert np.array_equal(_bits(g), _bits(plain[k][r]) if r is not None else np.zeros_like(_bits(g))), (j, k)


@pytest.mark.parametrize("index", ([0, 0, 3, 3, 3, 1], [6, 5, 4, 3, 2, 1, 0], [-1, 2, 4], [2, -1, -1, 4], [4, 2, -1],
                                   [-1, -1, -1], [-1, 7, 2, 100, -5]),
                         ids=("repeats", "descending", "front", "middle", "end", "all", "out_of_range"))
def test_index(dev, index):
    state, run, images, want = _case(3, 3, dev)
    d_maps = torch.from_numpy(images).to(dev)
    plain = _forward_guarded(dev, run, d_maps, len(images))
    got = _forward_guarded(dev, run, d_maps, len(index), index=index, chunk=2)
    for g, src in enumerate(index):
        if 0 <= src < len(images):
            assert _same_rows(got, g, plain, src), g
        else:
            assert all(not _bits(got[k][g]).any() for k in LEVELS), g


# ----------------------------------------------------------------------------------------------------------- invariance
def test_batch_run_and_chunk_invariance(dev):
    state, run, images, want = _case(12, 3, dev)
    full = GR.fixture_images(12)                                     # 33 images
    me = images[3]                                                   # a dense image
    alone = _call(run, torch.from_numpy(me[None]).to(dev))
    _check64(alone, want, slice(3, 4))
    for pos in (0, 16, 32):
        batch = full.copy()
        batch[pos] = me
        for chunk in (None, 5, 32):
            got = _call(run, torch.from_numpy(batch).to(dev), chunk=chunk)
            assert _same_rows(got, pos, alone, 0), (pos, chunk)
    nan_img = me.copy()
    nan_img[5, 30, 30] = np.nan
    for other in (np.zeros_like(me), me * np.float32(1e6), nan_img):
        for order in ((other, me), (me, other), (other, me, other)):
            got = _call(run, torch.from_numpy(np.stack(order)).to(dev))
            pos = [i for i, o in enumerate(order) if o is me][0]
            assert _same_rows(got, pos, alone, 0)
    d_full = torch.from_numpy(full).to(dev)
    runs = [_call(run, d_full) for _ in range(3)]
    assert _same_rows(runs[0], slice(None), runs[1], slice(None)) and _same_rows(runs[0], slice(None), runs[2],
                                                                                 slice(None))


# ----------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_pixels(dev, bad):
    state, run, images, want = _case(3, 3, dev)
    wide = np.concatenate([images, GR.hashed_images(len(images), 2, salt=9)], axis=1)           # 5 channels, 3 read
    plain = _forward_guarded(dev, run, torch.from_numpy(wide).to(dev), len(wide))
    _check64(plain, want)
    for ch, y, x in ((0, 0, 0), (2, 59, 59), (1, 31, 7)):
        hurt = wide.copy()
        hurt[2, ch, y, x] = bad
        got = _forward_guarded(dev, run, torch.from_numpy(hurt).to(dev), len(wide), chunk=3)
        assert np.isnan(got["logits"][2]).all()
        keep = [0, 1, 3, 4, 5, 6]
        assert _same_rows(got, keep, plain, keep)
    unread = wide.copy()
    unread[2, 3, 10, 10] = bad
    unread[4, 4, 0, 0] = bad
    got = _forward_guarded(dev, run, torch.from_numpy(unread).to(dev), len(wide))
    assert _same_rows(got, slice(None), plain, slice(None))


# ---------------------------------------------------------------------------------------------------------------- graph
def test_graph_replay_on_new_contents(dev):
    state, run, images, want = _case(12, 3, dev)
    other = np.ascontiguousarray(images[::-1])
    eager_a = _call(run, torch.from_numpy(images).to(dev))
    eager_b = _call(run, torch.from_numpy(other).to(dev))
    buf = torch.from_numpy(images).to(dev)
    idx = torch.arange(len(images), device=dev, dtype=torch.int32)
    run(buf, index=idx, features=True)                                # packs and warms up outside the capture
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        logits, f = run(buf, index=idx, features=True, chunk=3)
    outs = dict(f, logits=logits)
    for src, eager in ((other, eager_b), (images, eager_a)):
        buf.copy_(torch.from_numpy(src))
        for v in outs.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert _same_rows({k: v.cpu().numpy() for k, v in outs.items()}, slice(None), eager, slice(None))


# ----------------------------------------------------------------------------------------------------------- end to end
def test_score_projections_end_to_end(dev):
    from s4g_release_amd import postprocess as PP
    from tests import close_region_ref as CR
    fx = CR.load_fixture()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    labels = PP.label_baseline_view(t(fx["points"]), t(fx["frames"]), t(fx["cloud"]), t(fx["normals"]))
    state, run, _, _ = _case(12, 3, dev)
    run.pack(dev)
    torch.cuda.synchronize(dev)
    count = int(labels.best.count[0])
    F = labels.regions.maps.shape[1]
    assert count >= 20 and count < F
    vi = labels.best.valid_index[0].cpu().numpy()
    maps = labels.regions.maps[0].cpu().numpy()
    want = GR.forward64(state, maps[vi[:count]])["logits"]
    assert np.abs(want).max() > 0.1
    for grasp_num in (count - 3, count, count + 4, None):
        g = torch.cuda.CUDAGraph()                                    # a host sync inside would fail the capture
        with torch.cuda.graph(g):
            out = PP.score_projections(labels, run, grasp_num)
        g.replay()
        torch.cuda.synchronize(dev)
        K = F if grasp_num is None else min(grasp_num, F)
        assert tuple(out.shape) == (1, K, 3)
        got = out[0].cpu().numpy()
        n = min(K, count)
        assert GR.distance(got[:n], want[:n]) <= TOL * float(np.abs(want).max()) / float(np.abs(want[:n]).max())
        assert not _bits(got[n:]).any()
    every = PP.score_projections(labels.regions, run)
    torch.cuda.synchronize(dev)
    assert tuple(every.shape) == (1, F, 3)
    assert np.array_equal(_bits(every[0].cpu().numpy()[vi[:count]]), _bits(got[:count]))


# ---------------------------------------------------------------------------------------------------------- host checks
def test_host_checks_on_the_device(dev):
    from s4g_release_amd import _cabi
    state, run, images, want = _case(3, 3, dev)
    ok = torch.zeros(2, 3, 60, 60, device=dev)
    for bad in (ok.double(), ok.half(), ok[0], ok[:, :, :59], ok[:, :, :, :30], ok[:, :2], torch.zeros(2, 3, 64, 64, device=dev)):
        with pytest.raises(RuntimeError):
            run(bad)
    for bad_index in (torch.zeros(2, dtype=torch.int32), torch.zeros(2, device=dev), torch.zeros((1, 2), dtype=torch.int64, device=dev),
                      torch.zeros((1, 1, 1), dtype=torch.int64, device=dev)):
        with pytest.raises(RuntimeError):
            run(ok, index=bad_index)
    with pytest.raises(ValueError):
        run(ok, chunk=0)
    assert tuple(run(ok[:0]).shape) == (0, 3)
    lib = _cabi.lib()
    assert lib.s4g_gpd_pack_bytes(13, 3) == 0 and lib.s4g_gpd_pack_bytes(3, 17) == 0 and lib.s4g_gpd_pack_bytes(0, 3) == 0
    assert lib.s4g_gpd_workspace_bytes(3, 3, 3) < lib.s4g_gpd_workspace_bytes(4, 3, 3)
    assert lib.s4g_gpd_workspace_bytes(0, 3, 3) == lib.s4g_gpd_workspace_bytes(1024, 3, 3)
    d_maps = torch.from_numpy(images).to(dev)
    _forward_guarded(dev, run, d_maps, 9, expect=_cabi.S4G_EINVAL)                       # G > num_images without an index
    packed, logits = run.pack(dev), torch.zeros(7, 3, device=dev)
    ws = torch.zeros(int(lib.s4g_gpd_workspace_bytes(7, 3, 3)), dtype=torch.uint8, device=dev)
    args = lambda cin=3, K=3, chunk=0, nb=ws.numel(): (d_maps.data_ptr(), 3 * 3600, 3600, None, 7, 7, packed.data_ptr(),  # noqa: E731
                                                       cin, K, chunk, None, None, None, logits.data_ptr(), ws.data_ptr(), nb,
                                                       None)
    assert lib.s4g_gpd_forward_f32(*args(K=17)) == _cabi.S4G_EINVAL
    assert lib.s4g_gpd_forward_f32(*args(cin=0)) == _cabi.S4G_EINVAL
    assert lib.s4g_gpd_forward_f32(*args(chunk=-1)) == _cabi.S4G_EINVAL
    assert lib.s4g_gpd_forward_f32(*args(nb=ws.numel() - 1)) == _cabi.S4G_EWORKSPACE
