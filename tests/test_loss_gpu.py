"""GPU: the fused training objective and metric (csrc/loss.hip, s4g_release_amd/losses.py) against the fixture of the
reference's own classes and the float64 yardstick (tests/loss_ref.py; tests/test_loss_ref.py shows on the CPU what the
two can tell apart).  Every C-ABI call writes into guarded buffers and a guarded workspace.

Bounds (tests/loss_ref.py `bounds`): the kernel may be 4 x as far from float64 as the reference's own fp32 results in
the fixture are, losses with a floor of 2^-22 of the loss, gradients per element at the scale of the tensor's largest
magnitude; the rows whose sign branch fp32 cannot be held to are left out of the frame_R gradient (the CPU test caps
their share).  Measured distances: profiles/r29_loss.md."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loss_ref as LR

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -559038737
K = LR.kernel_constants()
T = K["LOSS_TILE"]
PRED_KEYS = {"score": "scene_score_logits", "mov": "movable_logits", "R": "frame_R", "t": "frame_t"}
LABEL_KEYS = {"y": "scene_score_labels", "mov_y": "scene_movable_labels", "best_R": "best_frame_R",
              "best_t": "best_frame_t", "scene_score": "scene_score"}
GRAD_OF = {"g_score": "score", "g_mov": "mov", "g_R": "R", "g_t": "t"}
ALL = ("g_score", "g_mov", "g_R", "g_t")


@pytest.fixture(scope="module")
def fx():
    return LR.load_fixture()


@pytest.fixture(scope="module")
def any_bounds(fx):
    """The bounds for inputs that are not the fixture's: the largest of its four cases."""
    return LR.bounds(fx)


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Call:
    """One prepared C-ABI call: device inputs, guarded outputs and workspace, the descriptor."""

    def __init__(self, dev, variant, preds, labels, ls=0.0, nw=0.1, grads=ALL, metric=False):
        from s4g_release_amd import _cabi
        self.dev, self.metric = dev, metric
        B, C, N = preds["score"].shape
        D, Ct, F = preds["mov"].shape[1], preds["t"].shape[1], labels["best_R"].shape[2]
        self.dims = (B, N, F, C, D, Ct)
        self.inputs = {k: _dev(v, dev) for k, v in list(preds.items()) + list(labels.items())}
        shapes = {"cls_acc": (B * N,), "mov_acc": (B * D * N,), "t_acc": (B * F,), "metrics": (2,)} if metric else \
            dict({"losses": (4,), "status": (1,)}, **{g: preds[GRAD_OF[g]].shape for g in grads})
        self.shapes = shapes
        self.bufs = {k: _guarded(s, dev) for k, s in shapes.items()}
        nbytes = int(_cabi.lib().s4g_grasp_loss_workspace_bytes(B, N, F))
        assert nbytes > 0
        self.nbytes = nbytes
        self.ws = torch.full((nbytes + 2 * GUARD * 4,), 0x5A, dtype=torch.uint8, device=dev)
        d = _cabi.LossDesc()
        d.variant, d.B, d.N, d.F, d.C, d.D, d.Ct = variant, B, N, F, C, D, Ct
        d.scene_score_stride = labels["scene_score"].shape[1]
        d.label_smoothing = ls
        d.w[0] = nw
        for c in range(1, C):
            d.w[c] = 1.0
        i = self.inputs
        d.score_logits, d.movable, d.frame_R, d.frame_t = (i[k].data_ptr() for k in ("score", "mov", "R", "t"))
        d.score_labels, d.movable_labels, d.best_frame_R, d.best_frame_t, d.scene_score = (
            i[k].data_ptr() for k in ("y", "mov_y", "best_R", "best_t", "scene_score"))
        names = {"g_mov": "g_movable"}
        for k, (_, view) in self.bufs.items():
            setattr(d, names.get(k, k), view.data_ptr())
        d.ws, d.ws_bytes = self.ws[GUARD * 4:].data_ptr(), nbytes
        self.d = d

    def launch(self, expect=0):
        from s4g_release_amd import _cabi
        from s4g_release_amd import functions as Fn
        fn = _cabi.lib().s4g_grasp_metric_f32 if self.metric else _cabi.lib().s4g_grasp_loss_f32
        with torch.cuda.device(self.dev):
            rc = fn(ctypes.byref(self.d), Fn._stream())
        assert rc == expect, rc

    def results(self):
        torch.cuda.synchronize(self.dev)
        for k, (buf, _) in self.bufs.items():
            assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "guard of %s" % k
        assert (self.ws[:GUARD * 4] == 0x5A).all() and (self.ws[GUARD * 4 + self.nbytes:] == 0x5A).all(), "workspace guard"
        out = {}
        for k, (_, view) in self.bufs.items():
            a = view.cpu().numpy()
            out[k] = a.reshape(self.shapes[k]) if k == "status" else a.view(np.float32).reshape(self.shapes[k])
        return out


def _abi(dev, variant, preds, labels, ls=0.0, nw=0.1, grads=ALL, metric=False):
    call = _Call(dev, variant, preds, labels, ls, nw, grads, metric)
    call.launch()
    return call.results()


def _check_loss(got, want, bl, bg, keep, scales=None, what=""):
    """The losses within bl of their scale (NaN where the yardstick has NaN) and every stored gradient within bg."""
    scales = np.abs(want["losses"]) if scales is None else scales
    for i in range(4):
        if np.isnan(want["losses"][i]):
            assert np.isnan(got["losses"][i]), (what, i, got["losses"])
        else:
            err = abs(float(got["losses"][i]) - want["losses"][i])
            assert err <= bl[i] * scales[i], (what, "loss", i, err, bl[i] * scales[i])
    dl, dg = LR.distances(got["losses"], got, want, keep)
    for name, dist in dg.items():
        assert dist <= bg[name], (what, name, dist, bg[name])
    return dl, dg


def _check_metric(fx, got, variant, preds, labels, what=""):
    want = LR.metric(variant, preds, labels)
    assert np.array_equal(got["cls_acc"], want["cls_acc"]), what
    assert np.array_equal(got["mov_acc"], want["mov_acc"]), what
    F = labels["best_R"].shape[2]
    if F == 0:
        assert np.isnan(got["metrics"][0]), what
        return
    rel_R, rel_t = _metric_rels(fx)
    bound = LR.r_err_bound(preds, labels, want, rel_R, LR.trace_eps(fx))
    assert abs(float(got["metrics"][0]) - want["R_err"]) <= bound, (what, got["metrics"], want["R_err"], bound)
    if variant == LR.CURVATURE:
        assert np.array_equal(got["t_acc"], want["t_acc"]), what
    else:
        assert abs(float(got["metrics"][1]) - want["t_err"]) <= rel_t * want["t_err"], (what, got["metrics"])


_RELS = []


def _metric_rels(fx):
    """The relative bounds of R_err and t_err: RULE x the fixture's own distance from float64, floor LOSS_FLOOR."""
    if not _RELS:
        d_R, d_t = [], []
        for tag, variant in LR.VARIANT_TAGS:
            _, p, lab, _, _ = LR.fixture_case(fx, tag, "ls0")
            m = LR.metric(variant, p, lab)
            d_R.append(abs(float(fx[tag + "/metric/R_err"]) - m["R_err"]) / m["R_err"])
            if variant == LR.CONTACT:
                d_t.append(abs(float(fx[tag + "/metric/t_err"]) - m["t_err"]) / m["t_err"])
        _RELS.extend([max(LR.RULE * max(d_R), LR.LOSS_FLOOR), max(LR.RULE * max(d_t), LR.LOSS_FLOOR)])
    return _RELS


# ---------------------------------------------------------------------------------------------------- fixture parity
CASES = [(tag, ls_tag) for tag, _ in LR.VARIANT_TAGS for ls_tag in LR.SMOOTHING_TAGS]


@pytest.mark.parametrize("tag,ls_tag", CASES)
def test_fixture_parity_through_the_c_abi(dev, fx, tag, ls_tag):
    variant, preds, labels, ls, nw = LR.fixture_case(fx, tag, ls_tag)
    want = LR.loss(variant, preds, labels, ls, nw)
    bl, bg = LR.bounds(fx, (tag, ls_tag))
    got = _abi(dev, variant, preds, labels, ls, nw)
    keep = LR.kept_mask(preds, labels, LR.branch_eps(fx))
    ref = LR.fixture_distances(fx)[tag, ls_tag]
    dl, dg = LR.distances(got["losses"], got, want, keep)
    print("%s/%s distance from float64: losses kernel %s reference %s; gradients kernel %s reference %s"
          % (tag, ls_tag, dl, ref[0], dg, ref[1]))
    _check_loss(got, want, bl, bg, keep, what=(tag, ls_tag))
    assert got["status"][0] == 0
    # the rows the gradient comparison leaves out are still one of the two branches
    und = ~keep[:, 0, :labels["best_R"].shape[2]]
    if und.any():
        other = LR.loss(variant, preds, labels, ls, nw, sabotage="max_for_min")
        e = np.minimum(np.abs(got["g_R"] - want["g_R"]), np.abs(got["g_R"] - other["g_R"]))
        assert e.max() <= bg["g_R"] * np.abs(want["g_R"]).max()
    if ls_tag == "ls0":
        _check_metric(fx, _abi(dev, variant, preds, labels, metric=True), variant, preds, labels, what=tag)


@pytest.mark.parametrize("tag,ls_tag", CASES)
def test_fixture_parity_through_the_modules(dev, fx, tag, ls_tag):
    from s4g_release_amd import losses
    variant, preds, labels, ls, nw = LR.fixture_case(fx, tag, ls_tag)
    want = LR.loss(variant, preds, labels, ls, nw)
    bl, bg = LR.bounds(fx, (tag, ls_tag))
    cls = losses.PointNet2Loss if variant == LR.CURVATURE else losses.ContactPointNet2Loss
    p = {PRED_KEYS[k]: _dev(v, dev).requires_grad_() for k, v in preds.items()}
    if variant == LR.CURVATURE:
        p["score"] = p.pop("scene_score_logits")                     # what the curvature network returns
    lab = {LABEL_KEYS[k]: _dev(v, dev) for k, v in labels.items()}   # scene_score is wider than F: its stride is passed
    loss = cls(label_smoothing=ls, neg_weight=nw)
    out = loss(p, lab)
    assert list(out) == ["cls_loss", "R_loss", "t_loss", "mov_loss"]
    sum(out.values()).backward()
    got = {"losses": np.array([float(out[k].detach()) for k in out], np.float32)}
    score_key = "score" if variant == LR.CURVATURE else "scene_score_logits"
    for g, k in (("g_score", score_key), ("g_mov", "movable_logits"), ("g_R", "frame_R"), ("g_t", "frame_t")):
        got[g] = p[k].grad.cpu().numpy()
    _check_loss(got, want, bl, bg, LR.kept_mask(preds, labels, LR.branch_eps(fx)), what=(tag, ls_tag))
    assert loss.status.is_cuda and int(loss.status) == 0
    # reweighting: the incoming scalars scale the unit gradients
    for v in p.values():
        v.grad = None
    out = loss(p, lab)
    (3.0 * out["R_loss"] - 0.5 * out["mov_loss"]).backward()
    assert torch.equal(p["frame_R"].grad, torch.from_numpy(got["g_R"]).to(dev) * 3.0)
    assert torch.equal(p["movable_logits"].grad, torch.from_numpy(got["g_mov"]).to(dev) * -0.5)
    assert p[score_key].grad is None or not p[score_key].grad.any()
    if ls_tag == "ls0":
        mcls = losses.PointNet2Metric if variant == LR.CURVATURE else losses.ContactPointNet2Metric
        m = mcls()(p, lab)
        got_m = {"cls_acc": m["cls_acc"].cpu().numpy(), "mov_acc": m["mov_acc"].cpu().numpy(),
                 "metrics": np.array([float(m["R_err"]), float(m.get("t_err", 0.0))], np.float32)}
        if "t_acc" in m:
            got_m["t_acc"] = m["t_acc"].cpu().numpy()
        assert ("t_acc" in m) == (variant == LR.CURVATURE) and ("t_err" in m) == (variant == LR.CONTACT)
        _check_metric(fx, got_m, variant, preds, labels, what=tag)


# -------------------------------------------------------------------------------------------------------- edge ladder
def _ladder():
    """(id, variant, B, N, F, C, D, Ct, ls, extra stride, gradient set): a curated list, not the product."""
    cases = []
    cs, ds, cts, bs = (2, 3, 8), (1, 5, 8), (2, 4, 8), (1, 3)
    i = 0
    for N in (1, 3, 4, 5, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        fs = sorted({0, 1, N - 1, N} & set(range(N + 1)))
        if N == 2 * T + 1:
            fs += [T - 1, T, T + 1]
        for F in fs:
            cases.append(("N%d-F%d" % (N, F), i % 2, bs[i % 2], N, F, cs[i % 3], ds[(i // 2) % 3], cts[(i // 3) % 3],
                          0.1 if i % 4 == 3 else 0.0, 0 if i % 3 else 5, ALL))
            i += 1
    for N in (5, 63, T - 1, T + 1, 2 * T + 1):          # N % 4 != 0 with every C: no vector access may start off alignment
        for C in cs:
            cases.append(("odd-N%d-C%d" % (N, C), C % 2, 3, N, N // 2, C, ds[C % 3], cts[C % 3], 0.0, 1, ALL))
    for N in (64, 65, T):                               # NULL gradient pointers: one at a time and all at once
        for k, name in enumerate(ALL):
            cases.append(("N%d-no-%s" % (N, name), k % 2, 2, N, N - 3, 3, 5, 4, 0.0, 0, tuple(g for g in ALL if g != name)))
        cases.append(("N%d-no-gradient" % N, 1, 2, N, N - 3, 3, 5, 4, 0.0, 2, ()))
    return cases


LADDER = _ladder()


@pytest.mark.parametrize("case", LADDER, ids=[c[0] for c in LADDER])
def test_edge_ladder_against_float64(dev, fx, any_bounds, case):
    name, variant, B, N, F, C, D, Ct, ls, extra, grads = case
    preds, labels = LR.random_case(len(name) * 1000 + N + F, variant, B, N, F, C, D, Ct, stride=F + extra)
    want = LR.loss(variant, preds, labels, ls, 0.5)
    got = _abi(dev, variant, preds, labels, ls, 0.5, grads=grads)
    assert sorted(k for k in got if k.startswith("g_")) == sorted(grads)
    bl, bg = any_bounds
    _check_loss(got, want, bl, bg, LR.kept_mask(preds, labels, LR.branch_eps(fx)),
                scales=LR.loss_scales(variant, preds, labels, want, 0.5), what=name)
    assert got["status"][0] == 0
    for g in ("g_R", "g_t"):                                          # nothing past the frame points
        assert g not in got or not got[g][:, :, F:].any(), (name, g)
    if grads == ALL:
        _check_metric(fx, _abi(dev, variant, preds, labels, metric=True), variant, preds, labels, what=name)


def test_every_label_ignored_and_no_frames(dev):
    preds, labels = LR.random_case(5, LR.CURVATURE, 2, 70, 9)
    labels["y"][:] = LR.IGNORE
    labels["best_t"][:] = LR.IGNORE
    got = _abi(dev, LR.CURVATURE, preds, labels)
    assert np.isnan(got["losses"][0]) and np.isnan(got["losses"][2]) and np.isfinite(got["losses"][[1, 3]]).all()
    assert not got["g_score"].any() and not got["g_t"].any() and got["g_R"].any() and got["status"][0] == 0
    for variant in (LR.CURVATURE, LR.CONTACT):
        preds, labels = LR.random_case(6, variant, 2, 70, 0)
        got = _abi(dev, variant, preds, labels)
        assert np.isnan(got["losses"][[1, 2]]).all() and np.isfinite(got["losses"][[0, 3]]).all()
        assert not got["g_R"].any() and not got["g_t"].any() and got["g_score"].any()


def test_refusals_leave_the_outputs_untouched(dev):
    from s4g_release_amd import _cabi
    preds, labels = LR.random_case(7, LR.CURVATURE, 2, 40, 10)
    for field, value, rc in (("C", 1, _cabi.S4G_EINVAL), ("C", 9, _cabi.S4G_EINVAL), ("D", 0, _cabi.S4G_EINVAL),
                             ("Ct", 9, _cabi.S4G_EINVAL), ("F", 41, _cabi.S4G_EINVAL), ("scene_score_stride", 9, _cabi.S4G_EINVAL),
                             ("B", 0, _cabi.S4G_EINVAL), ("B", 65536, _cabi.S4G_EINVAL), ("N", 2 ** 30, _cabi.S4G_EINVAL),
                             ("variant", 2, _cabi.S4G_EINVAL), ("label_smoothing", 1.0, _cabi.S4G_EINVAL),
                             ("score_logits", None, _cabi.S4G_EINVAL), ("losses", None, _cabi.S4G_EINVAL),
                             ("ws_bytes", 8, _cabi.S4G_EWORKSPACE), ("ws", None, _cabi.S4G_EWORKSPACE)):
        call = _Call(dev, LR.CURVATURE, preds, labels)
        setattr(call.d, field, value)
        call.launch(expect=rc)
        if field == "losses":
            call.bufs.pop("losses")
        torch.cuda.synchronize(dev)
        for k, (buf, _) in call.bufs.items():
            assert (buf == SENTINEL).all(), (field, k)
    call = _Call(dev, LR.CONTACT, *LR.random_case(8, LR.CONTACT, 1, 40, 10))
    call.d.Ct = 4
    call.launch(expect=_cabi.S4G_EINVAL)


# ------------------------------------------------------------------------------------------------------- exact family
def _dyadic_case(variant, B, N, F, seed=0):
    """Predictions and labels on which every L1, squared and min term is exact in fp32: multiples of 1/8 in [-2, 2],
    scores multiples of 1/16.  Rows 0-3: the zero label frame; rows 4-7: predictions with zero columns 1 and 2 (both
    exact ties); movable points 0-9: p == y."""
    rng = np.random.default_rng(seed)
    preds, labels = LR.random_case(seed, variant, B, N, F)

    def q(shape):
        return (rng.integers(-16, 17, shape) / 8.0).astype(np.float32)
    preds["R"], labels["best_R"] = q(preds["R"].shape), q(labels["best_R"].shape)
    labels["best_R"][:, :, 0:4] = 0
    preds["R"][:, [1, 2, 4, 5, 7, 8], 4:8] = 0
    labels["scene_score"] = (rng.integers(0, 17, labels["scene_score"].shape) / 16.0).astype(np.float32)
    labels["scene_score"][:, :8] = 0.5
    preds["mov"], labels["mov_y"] = (np.abs(q(preds["mov"].shape)) / 2).astype(np.float32), labels["mov_y"]
    preds["mov"][:, :, :10] = labels["mov_y"][:, :, :10]
    if variant == LR.CONTACT:
        preds["t"], labels["best_t"] = q(preds["t"].shape), q(labels["best_t"].shape)
    return preds, labels


@pytest.mark.parametrize("variant", [LR.CURVATURE, LR.CONTACT])
@pytest.mark.parametrize("N,F", [(T + 4, T + 1), (67, 40)])
def test_exact_family_is_the_yardstick_bit_for_bit(dev, variant, N, F):
    B = 2
    preds, labels = _dyadic_case(variant, B, N, F, seed=N)
    want = LR.loss(variant, preds, labels, 0.0, 0.5)
    L1, L2 = LR.r_branches(preds, labels)
    assert (L1[:, :8] == L2[:, :8]).all() and not want["second"][:, :8].any()
    got = _abi(dev, variant, preds, labels, 0.0, 0.5)
    exact = (1, 2, 3) if variant == LR.CONTACT else (1, 3)
    for i in exact:
        assert got["losses"][i] == np.float32(want["losses"][i]), (i, got["losses"], want["losses"])
    names = ("g_R", "g_mov", "g_t") if variant == LR.CONTACT else ("g_R", "g_mov")
    for name in names:
        assert np.array_equal(got[name], want[name].astype(np.float32)), name
    # the ties took branch 1: on rows 4-7 the two branches' gradients differ, and the kernel's is the first
    other = LR.loss(variant, preds, labels, 0.0, 0.5, sabotage="tie_branch2")["g_R"].astype(np.float32)
    assert (other[:, :, 4:8] != got["g_R"][:, :, 4:8]).any(axis=1).all()
    assert not got["g_mov"][:, :, :10].any()                         # p == y: sign(0) = 0


# -------------------------------------------------------------------------------------------------------------- status
def test_labels_outside_their_range_set_status_and_nothing_else(dev):
    preds, labels = LR.random_case(11, LR.CURVATURE, 2, T + 9, 77)
    C, Ct = preds["score"].shape[1], preds["t"].shape[1]
    clean = {k: v.copy() for k, v in labels.items()}
    spots = [(0, 0), (0, 5), (1, T), (1, T + 8)]
    for key in ("y", "best_t"):
        for b, n in spots:
            clean[key][b, n % clean[key].shape[1]] = LR.IGNORE
    base = _abi(dev, LR.CURVATURE, preds, clean, 0.0, 0.5)
    assert base["status"][0] == 0
    for key, bit, top in (("y", 1, C), ("best_t", 2, Ct)):
        bad = {k: v.copy() for k, v in clean.items()}
        for (b, n), v in zip(spots, (LR.IGNORE, top, -1, 2 ** 40)):
            bad[key][b, n % bad[key].shape[1]] = v
        got = _abi(dev, LR.CURVATURE, preds, bad, 0.0, 0.5)
        assert got["status"][0] == bit
        for k in base:
            if k != "status":
                assert np.array_equal(got[k].view(np.int32), base[k].view(np.int32)), (key, k)
    both = {k: v.copy() for k, v in clean.items()}
    both["y"][0, 0], both["best_t"][1, 3] = C, Ct
    assert _abi(dev, LR.CURVATURE, preds, both, 0.1, 0.5)["status"][0] == 3


# ----------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("variant", [LR.CURVATURE, LR.CONTACT])
def test_non_finite_predictions_touch_only_their_own_point(dev, variant):
    preds, labels = LR.random_case(13, variant, 2, T + 6, 50, ignore=0.0)
    base = _abi(dev, variant, preds, labels, 0.0, 0.5)
    spots = {"score": (0, 1, 7), "mov": (1, 2, T + 1), "R": (0, 4, 3), "t": (1, 0, 9)}
    for value in (np.nan, np.inf):
        bad = {k: v.copy() for k, v in preds.items()}
        for k, at in spots.items():
            bad[k][at] = value
        got = _abi(dev, variant, bad, labels, 0.0, 0.5)
        assert got["status"][0] == 0
        for g, k in GRAD_OF.items():
            b, _, n = spots[k]
            same = got[g].view(np.int32) == base[g].view(np.int32)
            same[b, :, n] = True
            assert same.all(), (value, g)
            assert not np.isfinite(got[g][b, :, n]).all() or g == "g_mov", (value, g)
        assert not np.isfinite(got["losses"]).all()


# ----------------------------------------------------------------------------------------------------------- run to run
@pytest.mark.parametrize("variant,N", [(LR.CURVATURE, 2 * T + 3), (LR.CONTACT, 2 * T + 4)])
def test_results_are_bit_identical_run_to_run_and_in_a_replayed_graph(dev, variant, N):
    preds, labels = LR.random_case(17, variant, 3, N, T + 5)
    call = _Call(dev, variant, preds, labels, 0.0, 0.5)
    call.launch()
    first = call.results()
    for _ in range(2):
        for _, view in call.bufs.values():
            view.fill_(SENTINEL)
        call.launch()
        again = call.results()
        for k in first:
            assert np.array_equal(first[k].view(np.int32), again[k].view(np.int32)), k
    for _, view in call.bufs.values():
        view.fill_(SENTINEL)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # one branch, one stream
        call.launch()
    for _ in range(2):
        for _, view in call.bufs.values():
            view.fill_(SENTINEL)
        graph.replay()
        again = call.results()
        for k in first:
            assert np.array_equal(first[k].view(np.int32), again[k].view(np.int32)), k


def test_module_forward_is_capturable_and_never_reads_back(dev):
    from s4g_release_amd import losses
    preds, labels = LR.random_case(19, LR.CURVATURE, 2, 300, 100)
    p = {PRED_KEYS[k]: _dev(v, dev) for k, v in preds.items()}
    lab = {LABEL_KEYS[k]: _dev(v, dev) for k, v in labels.items()}
    loss = losses.PointNet2Loss(neg_weight=0.5)
    eager = torch.stack(list(loss(p, lab).values()))
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                 # a host read or a synchronisation would fail the capture
        out = torch.stack(list(loss(p, lab).values()))
        status = loss.status
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, eager) and int(status) == 0


# ----------------------------------------------------------------------------------------------------------- end to end
CFG = dict(score_classes=3, num_centroids=(256, 64, 16), radius=(0.08, 0.2, 0.5), num_neighbours=(16, 16, 16),
           sa_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128)), fp_channels=((128, 128), (64, 64), (32, 32, 32)),
           num_fp_neighbours=(3, 3, 3), seg_channels=(64, 32, 32, 16), num_removal_directions=5, dropout_prob=0.0)
E2E = {"PN2_CLS": LR.CURVATURE, "PN2": LR.CONTACT}
E2E_N, E2E_F = 2048, 256
E2E_LR = 0.02           # measured: six steps take the total from 2.83 to about 2.69 (PN2_CLS), from 2.82 to about 2.50 (PN2)


def _setup(dev, model_type, seed=0):
    """The small network in train mode, two scenes, and labels of the real kinds: integer classes with holes,
    orthonormal frames, translation classes / points near the cloud, scores in [0, 1].  One label frame per scene (its
    sign branch drawn per point): frames drawn per point independently of the cloud leave a rotation head nothing to
    learn -- against uniformly random rotations every predicted rotation has the same expected min(L1, L2), and
    measured, R_loss then only wanders (1.107 -> 1.143 in six steps at any step size)."""
    from s4g_release_amd import synth
    from s4g_release_amd.model import MODEL_TYPES
    torch.manual_seed(seed)
    net = MODEL_TYPES[model_type](**CFG).to(dev).train()
    pts = synth.make_batch([1, 2], E2E_N)
    _, labels = LR.random_case(seed + 1, E2E[model_type], 2, E2E_N, E2E_F, stride=E2E_F + 8)
    rng = np.random.default_rng(seed + 2)
    flip = np.where(rng.random((2, 1, E2E_F)) < 0.5, LR.NEG[None, :, None], 1.0)
    labels["best_R"] = (LR.rotations(rng, (2,)).reshape(2, 9, 1) * flip).astype(np.float32)
    if E2E[model_type] == LR.CONTACT:
        labels["best_t"] = (pts[:, :, :E2E_F] + 0.02 * rng.standard_normal((2, 3, E2E_F))).astype(np.float32)
    lab = {LABEL_KEYS[k]: _dev(v, dev) for k, v in labels.items()}
    return net, torch.from_numpy(pts).to(dev), lab


def _torch_constants(classes, neg_weight, dev):
    """(class weights, sign of the second branch): made by host writes, as the reference makes its weights in every
    forward -- which a graph capture refuses, so tools/bench_loss.py makes them once, outside."""
    w = torch.ones(classes, device=dev)
    w[0] = neg_weight
    return w, torch.tensor([1.0, -1.0, -1.0] * 3, device=dev).view(1, 9, 1)


def _torch_loss(variant, pred, lab, neg_weight, constants=None):
    """The objective restated in plain torch operations, for the gradients of a whole step."""
    import torch.nn.functional as TF
    score = pred["score"] if "score" in pred else pred["scene_score_logits"]
    w, flip = constants or _torch_constants(score.shape[1], neg_weight, score.device)
    out = {"cls_loss": TF.cross_entropy(score, lab["scene_score_labels"], w),
           "mov_loss": (pred["movable_logits"] - lab["scene_movable_labels"]).abs().mean()}
    g = lab["best_frame_R"]
    F = g.shape[2]
    s = lab["scene_score"][:, :F]
    p = pred["frame_R"][:, :, :F]
    both = torch.stack([((p - g) ** 2).mean(1), ((p - g * flip) ** 2).mean(1)], 1)
    out["R_loss"] = (both.min(1)[0] * s).mean() * 5.0
    t = pred["frame_t"][:, :, :F]
    if variant == LR.CURVATURE:
        out["t_loss"] = TF.cross_entropy(t, lab["best_frame_t"]) * 0.2
    else:
        out["t_loss"] = (((t - lab["best_frame_t"]) ** 2).sum(1) * s).mean() * 20.0
    return out


def _step_grads(dev, model_type, fused, seed=3):
    import s4g_release_amd as S
    net, pts, lab = _setup(dev, model_type, seed)
    pred = net({"scene_points": pts})
    loss = S.build_loss(model_type)[0](pred, lab) if fused else _torch_loss(E2E[model_type], pred, lab, 0.5)
    sum(loss.values()).backward()
    return {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("model_type", sorted(E2E))
def test_sgd_steps_on_the_fused_loss_lower_it(dev, model_type):
    import s4g_release_amd as S
    from s4g_release_amd import functions as F
    F.set_backward_mode("deterministic")
    net, pts, lab = _setup(dev, model_type)
    loss_fn, metric_fn = S.build_loss(model_type)
    opt = torch.optim.SGD(net.parameters(), lr=E2E_LR, momentum=0.0)
    totals = []
    for step in range(6):
        opt.zero_grad()
        pred = net({"scene_points": pts})
        loss = loss_fn(pred, lab)
        total = sum(loss.values())
        total.backward()
        if step == 0:
            # the contact network's t_logit starts at zero (reference PointNet2.py:150-152): in the first step it
            # receives a gradient and passes none on to mlp_t
            named = [(n, p) for n, p in net.named_parameters()
                     if not (E2E[model_type] == LR.CONTACT and n.startswith("mlp_t."))]
            got = [n for n, p in named if p.grad is not None and p.grad.abs().max() > 0]
            assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
            assert len(got) >= 0.9 * len(named), "most parameters must receive a gradient"
            assert "t_logit.weight" in got and "seg_logit.weight" in got and "R_logit.weight" in got
        opt.step()
        totals.append(float(total.detach()))
    print(model_type, totals)
    assert np.isfinite(totals).all() and totals[-1] < totals[0], totals
    assert int(loss_fn.status) == 0
    m = metric_fn(pred, lab)
    assert m["cls_acc"].shape == (2 * E2E_N,) and bool(torch.isfinite(m["R_err"]))


@pytest.mark.parametrize("model_type", sorted(E2E))
def test_step_gradients_repeat_and_agree_with_the_plain_torch_loss(dev, model_type):
    from s4g_release_amd import functions as F
    was = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        F.set_backward_mode("deterministic")
        a, b = _step_grads(dev, model_type, True), _step_grads(dev, model_type, True)
        assert sorted(a) == sorted(b) and len(a) > 50
        for n in a:
            assert torch.equal(a[n], b[n]), n
        F.set_backward_mode("atomic")
        t1, t2 = _step_grads(dev, model_type, False), _step_grads(dev, model_type, False)
        gmax = max(float(g.abs().max()) for g in t1.values())
        spread = max(float((t1[n] - t2[n]).abs().max()) for n in t1)
        bound = max(4.0 * spread, 1e-5 * gmax)
        worst = max(float((a[n] - t1[n]).abs().max()) for n in t1)
        print("%s: largest gradient %.3g, torch spread %.3g, bound %.3g, fused against torch %.3g"
              % (model_type, gmax, spread, bound, worst))
        assert gmax > 0 and sorted(a) == sorted(t1)
        assert worst <= bound, (worst, bound)
    finally:
        F.set_backward_mode("deterministic")
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was
