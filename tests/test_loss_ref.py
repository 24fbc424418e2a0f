"""CPU: the float64 yardstick of the training objective (tests/loss_ref.py) against the fixture of the reference's own
classes (tests/golden/loss.npz, tools/gen_golden_loss.py); the sabotaged readings each seen; the decided share; the
constants of csrc/loss.hip; and the refusals of the host layer (s4g_release_amd/losses.py), which has no CPU path."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import loss_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/inference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
CASES = [(tag, ls_tag) for tag, _ in LR.VARIANT_TAGS for ls_tag in LR.SMOOTHING_TAGS]
# the distance of fp32 results from float64 that a handful of roundings explains: 16 x 2^-24
FP32_FEW = 16 * 2.0 ** -24


@pytest.fixture(scope="module")
def fx():
    return LR.load_fixture()


def test_fixture_holds_what_the_issue_asks_of_it(fx):
    for tag, variant in LR.VARIANT_TAGS:
        _, preds, labels, _, nw = LR.fixture_case(fx, tag, "ls0")
        B, C, N = preds["score"].shape
        F = labels["best_R"].shape[2]
        assert (B, C, N, F, preds["mov"].shape[1], nw) == (2, 3, 515, 300, 5, 0.5) and N % 4
        assert labels["scene_score"].shape[1] > F                              # a wider tensor is sliced
        assert (labels["y"] == LR.IGNORE).sum() >= 20 and (fx[tag + "/label/y_smooth"] >= 0).all()
        assert not labels["best_R"][:, :, :20].any() and (labels["scene_score"][:, :20] > 0).all()
        assert (labels["scene_score"][:, 40:70] == 0).all()
        assert (preds["mov"] == labels["mov_y"]).sum() >= 20
        L1, L2 = LR.r_branches(preds, labels)
        assert (L1[:, :20] == L2[:, :20]).all()
        if variant == LR.CURVATURE:
            assert (labels["best_t"] == LR.IGNORE).sum() >= 20
            assert (L1[:, 20:40] == L2[:, 20:40]).all() and labels["best_R"][:, 1, 20:40].all()
        else:                                                                  # true rotations
            m = preds["R"].astype(np.float64).reshape(B, 3, 3, N).transpose(0, 3, 1, 2)
            assert np.abs(m @ m.transpose(0, 1, 3, 2) - np.eye(3)).max() < 1e-5
            assert np.abs(np.linalg.det(m) - 1).max() < 1e-5


@pytest.mark.parametrize("tag,ls_tag", CASES)
def test_yardstick_reproduces_the_fixture(fx, tag, ls_tag):
    dl, dg = LR.fixture_distances(fx)[tag, ls_tag]
    print("%s/%s: losses %s gradients %s" % (tag, ls_tag, dl, dg))
    assert (dl < FP32_FEW).all(), dl
    assert all(v < FP32_FEW for v in dg.values()), dg


@pytest.mark.parametrize("tag", [t for t, _ in LR.VARIANT_TAGS])
def test_yardstick_reproduces_the_fixture_metrics(fx, tag):
    variant, preds, labels, _, _ = LR.fixture_case(fx, tag, "ls0")
    m = LR.metric(variant, preds, labels)
    assert np.array_equal(m["cls_acc"], fx[tag + "/metric/cls_acc"]) and 0.1 < m["cls_acc"].mean() < 0.9
    assert np.array_equal(m["mov_acc"], fx[tag + "/metric/mov_acc"]) and 0.1 < m["mov_acc"].mean() < 0.9
    assert abs(m["R_err"] - float(fx[tag + "/metric/R_err"])) < LR.r_err_bound(preds, labels, m, FP32_FEW,
                                                                               LR.trace_eps(fx) / LR.RULE)
    if variant == LR.CURVATURE:
        assert np.array_equal(m["t_acc"], fx[tag + "/metric/t_acc"]) and 0.05 < m["t_acc"].mean() < 0.9
    else:
        assert abs(m["t_err"] - float(fx[tag + "/metric/t_err"])) < FP32_FEW * m["t_err"]


def test_decided_share(fx):
    """At most 2 % of the F rows may be left out of the frame_R gradient comparison, and of the R_err rows as many may
    sit at the clamp."""
    eps, teps = LR.branch_eps(fx), LR.trace_eps(fx)
    assert 0 < eps < 1e-5 and 0 < teps < 1e-5
    for tag, _ in LR.VARIANT_TAGS:
        _, preds, labels, _, _ = LR.fixture_case(fx, tag, "ls0")
        und, clamp = LR.undecided_rows(preds, labels, eps), LR.clamp_rows(preds, labels, teps)
        print("%s: %d undecided branch rows, %d rows at the clamp, of %d" % (tag, und.sum(), clamp.sum(), und.size))
        assert und.mean() <= 0.02 and clamp.mean() <= 0.02


def _misses(fx, tag, ls_tag, sabotage):
    """Does the sabotaged reading miss case (tag, ls_tag) -- a loss, or at least 20 kept gradient rows -- by >= 100 x
    the bound?"""
    variant, preds, labels, ls, nw = LR.fixture_case(fx, tag, ls_tag)
    want, bad = LR.loss(variant, preds, labels, ls, nw), LR.loss(variant, preds, labels, ls, nw, sabotage=sabotage)
    bl, bg = LR.bounds(fx, (tag, ls_tag))
    if (np.abs(bad["losses"] - want["losses"]) >= 100 * bl * np.abs(want["losses"])).any():
        return True
    keep = LR.kept_mask(preds, labels, LR.branch_eps(fx))
    for name, _ in LR.GRADS:
        err = np.abs(bad[name] - want[name])
        if name == "g_R":
            err = np.where(keep, err, 0.0)
        rows = (err >= 100 * bg[name] * np.abs(want[name]).max()).any(axis=1)        # (B, N): a point is a row
        if rows.sum() >= 20:
            return True
    return False


@pytest.mark.parametrize("sabotage", LR.SABOTAGES)
def test_every_sabotage_is_seen(fx, sabotage):
    seen = [case for case in CASES if _misses(fx, case[0], case[1], sabotage)]
    print(sabotage, "seen by", seen)
    assert seen, sabotage


def test_tie_and_sign_sabotages_are_seen_in_the_gradient_rows_planted_for_them(fx):
    variant, preds, labels, ls, nw = LR.fixture_case(fx, "curv", "ls0")
    want = LR.loss(variant, preds, labels, ls, nw)
    tie = LR.loss(variant, preds, labels, ls, nw, sabotage="tie_branch2")
    assert np.array_equal(tie["losses"], want["losses"])                       # a tie: the loss cannot tell
    rows = (tie["g_R"] != want["g_R"]).any(axis=1)
    assert rows[:, 20:40].all() and rows.sum() == 40                           # the zero frame cannot tell either
    sign = LR.loss(variant, preds, labels, ls, nw, sabotage="sign0_is_1")
    assert ((sign["g_mov"] != want["g_mov"]).any(axis=1)).sum() >= 20


def test_kernel_constants_and_limits():
    from s4g_release_amd import losses
    k = LR.kernel_constants()
    assert k["LOSS_TILE"] == k["LOSS_THREADS"] * k["LOSS_PTS"] and k["LOSS_PTS"] == 4      # one float4 per channel
    assert k["LOSS_THREADS"] % 64 == 0 and k["LOSS_HIST_TILE"] % k["LOSS_THREADS"] == 0
    assert k["LOSS_MAX_CH"] == losses.MAX_CHANNELS == 8
    assert k["LOSS_MAX_B"] == losses.MAX_B == 65535 and k["LOSS_MAX_POINTS"] == 2 ** 31 - 1
    src = open(os.path.join(ROOT, "s4g_release_amd", "csrc", "loss.hip")).read()
    assert "atomicAdd(float" not in src.replace(" ", "") and "unsafeAtomicAdd" not in src


def test_workspace_query_follows_the_limits():
    from s4g_release_amd import _cabi
    k = LR.kernel_constants()
    ws = _cabi.lib().s4g_grasp_loss_workspace_bytes
    assert ws(1, 1, 0) > 0 and ws(2, 515, 300) > 0
    assert ws(0, 8, 0) == 0 and ws(1, 0, 0) == 0 and ws(1, 8, 9) == 0 and ws(1, 8, -1) == 0
    assert ws(k["LOSS_MAX_B"] + 1, 1, 0) == 0 and ws(k["LOSS_MAX_B"], 1, 0) > 0
    assert ws(2, 2 ** 30, 0) == 0 and ws(1, k["LOSS_MAX_POINTS"], 0) > 0
    # one more tile of points is one more row of partials
    assert ws(1, k["LOSS_TILE"] + 1, 0) - ws(1, k["LOSS_TILE"], 0) == 4 * 8


def _cpu_inputs(variant, B=2, N=12, F=5, **kw):
    preds, labels = LR.random_case(0, variant, B, N, F, **kw)
    p = {"scene_score_logits": preds["score"], "movable_logits": preds["mov"], "frame_R": preds["R"], "frame_t": preds["t"]}
    lab = {"scene_score_labels": labels["y"], "scene_movable_labels": labels["mov_y"], "best_frame_R": labels["best_R"],
           "best_frame_t": labels["best_t"], "scene_score": labels["scene_score"]}
    return ({k: torch.from_numpy(v) for k, v in p.items()}, {k: torch.from_numpy(v) for k, v in lab.items()})


@pytest.mark.parametrize("model_type,variant", [("PN2_CLS", LR.CURVATURE), ("PN2", LR.CONTACT), ("EDGEPN2D", LR.CONTACT)])
def test_cpu_tensors_and_bad_inputs_raise_value_error(model_type, variant):
    import s4g_release_amd as S
    loss, metric = S.build_loss(model_type)
    for fn in (loss, metric):
        p, lab = _cpu_inputs(variant)
        with pytest.raises(ValueError, match="CUDA tensor"):                   # the house rule: no CPU path
            fn(p, lab)
        p["score"] = p.pop("scene_score_logits")                               # either key names the score logits
        with pytest.raises(ValueError, match="CUDA tensor"):
            fn(p, lab)
        del p["score"]
        with pytest.raises(ValueError, match="scene_score_logits"):
            fn(p, lab)
        for key, bad, what in (
                ("frame_R", lambda t: t.double(), "frame_R must be torch.float32"),
                ("frame_R", lambda t: t[:, :8], "frame_R must have shape"),
                ("frame_t", lambda t: t[:, :, :-1], "frame_t must have shape"),
                ("movable_logits", lambda t: t.half(), "movable_logits must be torch.float32"),
                ("scene_score_logits", lambda t: t[:, :1], "2 to 8 classes"),
                ("scene_score_logits", lambda t: torch.cat([t, t, t], 1), "2 to 8 classes")):
            p, lab = _cpu_inputs(variant)
            p[key] = bad(p[key])
            with pytest.raises(ValueError, match=what):
                fn(p, lab)
        for key, bad, what in (
                ("scene_score_labels", lambda t: t.int(), "scene_score_labels must be torch.int64"),
                ("scene_score_labels", lambda t: t[:, :-1], "scene_score_labels must have shape"),
                ("scene_movable_labels", lambda t: t[:, :-1], "scene_movable_labels must have shape"),
                ("best_frame_R", lambda t: torch.cat([t, t, t], 2), "more than the 12 points"),
                ("best_frame_t", lambda t: t.to(torch.float64), "best_frame_t must be"),
                ("scene_score", lambda t: t[:, :-1], "fewer than the 5 frame points")):
            p, lab = _cpu_inputs(variant)
            lab[key] = bad(lab[key])
            if key == "best_frame_R":
                lab["best_frame_t"] = torch.cat([lab["best_frame_t"]] * 3, -1)
                lab["scene_score"] = torch.cat([lab["scene_score"]] * 3, -1)
            with pytest.raises(ValueError, match=what):
                fn(p, lab)
    p, lab = _cpu_inputs(variant)
    p["frame_t"] = torch.zeros(2, 9 if variant == LR.CURVATURE else 4, 12)
    with pytest.raises(ValueError, match="frame_t must have"):
        loss(p, lab)


def test_build_loss_covers_the_three_supported_types():
    import s4g_release_amd as S
    from s4g_release_amd import losses, model
    assert sorted(losses.LOSS_TYPES) == sorted(model.MODEL_TYPES)
    loss, metric = S.build_loss("PN2_CLS", label_smoothing=0.1)
    assert type(loss) is losses.PointNet2Loss and type(metric) is losses.PointNet2Metric
    assert (loss.label_smoothing, loss.neg_weight) == (0.1, 0.5)               # the shipped yaml value
    assert losses.PointNet2Loss().neg_weight == 0.1 and losses.PointNet2Loss().label_smoothing == 0
    for t in ("PN2", "EDGEPN2D"):
        loss, metric = S.build_loss(t, neg_weight=0.25)
        assert type(loss) is losses.ContactPointNet2Loss and type(metric) is losses.ContactPointNet2Metric
        assert loss.neg_weight == 0.25
    for t in ("PN2_LOCAL", "EDGEPN2DU", "GPD", ""):
        with pytest.raises(ValueError, match="unsupported MODEL.TYPE"):
            S.build_loss(t)
    with pytest.raises(ValueError, match="label_smoothing"):
        losses.PointNet2Loss(label_smoothing=1.0)
    assert callable(S.PointNet2Loss) and callable(S.ContactPointNet2Metric)


@needs_ref
def test_committed_loss_fixture_is_what_the_reference_classes_produce(tmp_path):
    """Provenance: tools/gen_golden_loss.py re-run here (child process) gives the committed fixture array for array."""
    code = "import sys; sys.path.insert(0, %r); from tools import gen_golden_loss as G; G.gen(%r)" % (ROOT, str(tmp_path))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    new, old = np.load(os.path.join(str(tmp_path), "loss.npz"), allow_pickle=False), LR.load_fixture()
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        if k.endswith("err"):                                                  # a measured fp32 error: its size
            assert 0.5 * old[k] <= new[k] <= 2.0 * old[k], k
        elif old[k].dtype.kind in "fc":
            assert np.allclose(new[k], old[k], rtol=0, atol=2e-6 * max(1e-30, float(np.abs(old[k]).max()))), k
        else:
            assert np.array_equal(new[k], old[k]), k
