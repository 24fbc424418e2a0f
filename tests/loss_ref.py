"""Float64 yardstick of the training objective and metric (`s4g_release_amd/losses.py`, `csrc/loss.hip`), written from the
statements of the reference's `PointNet2Loss` / `PointNet2Metric` (network_models/models/PointNet2_tcls.py:156-267, the
curvature variant 0; PointNet2.py:156-258, the contact variant 1) and `smooth_cross_entropy`
(nn_utils/functional.py:91-114): the four losses, the gradient of each with respect to its own prediction tensor, and
the metrics.  `SABOTAGES` names single wrong readings of those statements; `loss(..., sabotage=name)` computes that
reading instead, and tests/test_loss_ref.py shows that the fixture tells every one of them from the right one.

Shapes: preds = {"score" (B, C, N), "mov" (B, D, N), "R" (B, 9, N), "t" (B, Ct, N)}; labels = {"y" (B, N) int64,
"mov_y" (B, D, N), "best_R" (B, 9, F), "best_t" (B, F) int64 or (B, 3, F), "scene_score" (B, >= F)}."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVATURE, CONTACT = 0, 1
IGNORE = -100
NEG = np.array([1.0, -1.0, -1.0] * 3)            # the sign branch: columns 1 and 2 of the row-major frame negated
LOSS_FLOOR = 2.0 ** -22                          # of the loss: one final rounding at 2^-24 and the fp32 expf / logf
RULE = 4.0                                       # the kernel may be this many times as far from float64 as the fixture

SABOTAGES = (
    "plain_mean",             # cls: plain mean over the counted rows in place of the weighted mean
    "neg_weight_class1",      # cls: neg_weight on class 1 instead of class 0
    "rows_negated",           # R: rows 1-2 of the label frame negated instead of columns 1-2
    "max_for_min",            # R: the larger branch
    "tie_branch2",            # R: an exact tie takes the negated branch
    "n_for_f",                # R, t: the mean over B N instead of B F
    "no_scene_score",         # R, t (contact): scene_score dropped
    "no_factor",              # R, t: the factors 5 / 0.2 / 20 dropped
    "no_ls_over_c",           # smooth cls: the ls / C term dropped
    "smooth_weight_by_label", # smooth cls: w[y] in place of w_c
    "sign0_is_1",             # mov: sign(0) = 1
    "ignore_counted",         # cls, t (curvature): label -100 counted in the denominator
)


def kernel_constants():
    """The tile constants and limits of csrc/loss.hip, read out of the source."""
    src = open(os.path.join(ROOT, "s4g_release_amd", "csrc", "loss.hip")).read()
    out = {}
    for name in ("LOSS_THREADS", "LOSS_PTS", "LOSS_TILE", "LOSS_HIST_TILE", "LOSS_MAX_CH", "LOSS_MAX_B"):
        m = re.search(r"constexpr\s+(?:int|int64_t)\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m, "csrc/loss.hip no longer defines %s as a literal" % name
        out[name] = int(m.group(1))
    m = re.search(r"constexpr\s+int64_t\s+LOSS_MAX_POINTS\s*=\s*\(1ll\s*<<\s*(\d+)\)\s*-\s*1\s*;", src)
    assert m, "csrc/loss.hip no longer defines LOSS_MAX_POINTS as (1ll << k) - 1"
    out["LOSS_MAX_POINTS"] = (1 << int(m.group(1))) - 1
    return out


def _f64(d):
    return {k: (np.asarray(v).astype(np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v))
            for k, v in d.items()}


def _log_softmax(x):
    """over axis 1"""
    z = x - x.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def _cross_entropy(logits, y, w, counted_ignored=False):
    """torch's F.cross_entropy(logits (B, K, M), y (B, M), w): weighted mean, -100 and (decision 2) every other label
    outside [0, K) in neither sum.  -> (loss, gradient, denominator)"""
    B, K, M = logits.shape
    lp = _log_softmax(logits)
    ok = (y >= 0) & (y < K)
    yc = np.where(ok, y, 0)
    onehot = (np.arange(K)[None, :, None] == yc[:, None, :]) & ok[:, None, :]
    wy = np.where(ok, w[yc], 0.0)
    den = wy.sum() + (float((y == IGNORE).sum()) if counted_ignored else 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = -(wy * (lp * onehot).sum(axis=1)).sum() / den
        grad = wy[:, None, :] * (np.exp(lp) - onehot) * ok[:, None, :] / den
    return loss, np.where(ok[:, None, :], grad, 0.0), den


def r_branches(preds, labels):
    """(L1, L2) of the first F points, (B, F) each: mean_9 (p - g)^2 against the label frame and its sign branch."""
    p, g = _f64(preds)["R"], _f64(labels)["best_R"]
    F = g.shape[2]
    p = p[:, :, :F]
    return ((p - g) ** 2).mean(axis=1), ((p - g * NEG[None, :, None]) ** 2).mean(axis=1)


def loss(variant, preds, labels, label_smoothing=0.0, neg_weight=0.1, sabotage=None):
    """-> {"losses": (4,) cls R t mov, "g_score", "g_mov", "g_R", "g_t": unit gradients, "second": (B, F) bool, the rows
    that took the negated branch}"""
    assert sabotage is None or sabotage in SABOTAGES, sabotage
    P, L = _f64(preds), _f64(labels)
    score, mov, R, t = P["score"], P["mov"], P["R"], P["t"]
    y, mov_y, best_R, best_t, scene = L["y"], L["mov_y"], L["best_R"], L["best_t"], L["scene_score"]
    B, C, N = score.shape
    F = best_R.shape[2]
    w = np.ones(C)
    w[1 if sabotage == "neg_weight_class1" else 0] = neg_weight
    out = {}
    # ---- cls
    if label_smoothing > 0:
        lp = _log_softmax(score)
        ok = (y >= 0) & (y < C)
        onehot = (np.arange(C)[None, :, None] == y[:, None, :]).astype(np.float64)
        s = onehot * (1 - label_smoothing) + (0.0 if sabotage == "no_ls_over_c" else label_smoothing / C)
        wc = w[np.where(ok, y, 0)][:, None, :] * np.ones((1, C, 1)) if sabotage == "smooth_weight_by_label" \
            else w[None, :, None] * np.ones((B, 1, N))
        s = s * ok[:, None, :]
        cls = -(s * lp * wc).sum() / (B * N)
        g_score = ((s * wc).sum(axis=1, keepdims=True) * np.exp(lp) - s * wc) / (B * N)
    else:
        cls, g_score, den = _cross_entropy(score, y, w, counted_ignored=sabotage == "ignore_counted")
        if sabotage == "plain_mean":
            count = float(((y >= 0) & (y < C)).sum())
            cls, g_score = cls * den / count, g_score * den / count
    # ---- mov
    diff = mov - mov_y
    sign = np.sign(diff)
    if sabotage == "sign0_is_1":
        sign = np.where(diff == 0, 1.0, sign)
    g_mov = sign / diff.size
    movl = np.abs(diff).mean()
    # ---- R
    neg = np.array([1.0] * 3 + [-1.0] * 6) if sabotage == "rows_negated" else NEG
    pR = R[:, :, :F]
    g2 = best_R * neg[None, :, None]
    L1, L2 = ((pR - best_R) ** 2).mean(axis=1), ((pR - g2) ** 2).mean(axis=1)
    second = L2 < L1
    if sabotage == "max_for_min":
        second = L2 > L1
    if sabotage == "tie_branch2":
        second = L2 <= L1
    sc = np.ones((B, F)) if sabotage == "no_scene_score" else scene[:, :F]
    kR = 1.0 if sabotage == "no_factor" else 5.0
    den_f = float(B * (N if sabotage == "n_for_f" else F))
    with np.errstate(invalid="ignore", divide="ignore"):
        Rl = (np.where(second, L2, L1) * sc).sum() / den_f * kR
        gsel = np.where(second[:, None, :], g2, best_R)
        g_R = np.zeros_like(R)
        if F:
            g_R[:, :, :F] = kR * sc[:, None, :] * 2.0 * (pR - gsel) / 9.0 / den_f
    # ---- t
    g_t = np.zeros_like(t)
    if variant == CURVATURE:
        kT = 1.0 if sabotage == "no_factor" else 0.2
        tl, gt, den = _cross_entropy(t[:, :, :F], best_t, np.ones(t.shape[1]), counted_ignored=sabotage == "ignore_counted")
        if sabotage == "n_for_f":
            tl, gt = tl * den / (B * N), gt * den / (B * N)
        tl = tl * kT
        if F:
            g_t[:, :, :F] = gt * kT
    else:
        kT = 1.0 if sabotage == "no_factor" else 20.0
        dt = t[:, :, :F] - best_t
        with np.errstate(invalid="ignore", divide="ignore"):
            tl = ((dt ** 2).sum(axis=1) * sc).sum() / den_f * kT
            if F:
                g_t[:, :, :F] = kT * sc[:, None, :] * 2.0 * dt / den_f
    out.update(losses=np.array([cls, Rl, tl, movl]), g_score=g_score, g_mov=g_mov, g_R=g_R, g_t=g_t, second=second)
    return out


def undecided_rows(preds, labels, eps):
    """(B, F) bool: the rows whose branch fp32 arithmetic cannot be held to -- |L1 - L2| <= eps (L1 + L2), except the
    exact ties (decision 1 pins those)."""
    L1, L2 = r_branches(preds, labels)
    return (np.abs(L1 - L2) <= eps * (L1 + L2)) & (L1 != L2)


def traces(preds, labels):
    """((tr1 - 1) / 2, (tr2 - 1) / 2) of the metric, (B, F) each, before the clamp."""
    p, g = _f64(preds)["R"], _f64(labels)["best_R"]
    F = g.shape[2]
    p = p[:, :, :F]
    return ((g * p).sum(axis=1) - 1.0) / 2.0, ((g * NEG[None, :, None] * p).sum(axis=1) - 1.0) / 2.0


def metric(variant, preds, labels):
    """-> {"cls_acc" (B N,), "mov_acc" (B D N,), "R_err", "R_rows" (B, F) the per-point terms, "t_acc" (B F,) | "t_err"}"""
    P, L = _f64(preds), _f64(labels)
    B, C, N = P["score"].shape
    F = L["best_R"].shape[2]
    out = {"cls_acc": (P["score"].argmax(axis=1) == L["y"]).reshape(-1).astype(np.float64),
           "mov_acc": ((P["mov"] > 0.5).astype(np.int64) == L["mov_y"].astype(np.int64)).reshape(-1).astype(np.float64)}
    c1, c2 = traces(preds, labels)
    a = np.minimum(np.arccos(np.clip(c1, -1.0, 1.0)), np.arccos(np.clip(c2, -1.0, 1.0)))
    rows = L["scene_score"][:, :F] * a
    with np.errstate(invalid="ignore", divide="ignore"):
        out["R_rows"], out["R_err"] = rows, rows.sum() / float(B * F)
        if variant == CURVATURE:
            out["t_acc"] = (P["t"][:, :, :F].argmax(axis=1) == L["best_t"]).reshape(-1).astype(np.float64)
        else:
            out["t_err"] = np.sqrt(((L["best_t"] - P["t"][:, :, :F]) ** 2).sum(axis=1)).sum() / float(B * F)
    return out


# ------------------------------------------------------------------------------------------------------- random inputs
def rotations(rng, shape):
    """random rotation matrices, (*shape, 3, 3) float64"""
    q, r = np.linalg.qr(rng.standard_normal(shape + (3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[..., None, :]
    q[..., :, 2] *= np.linalg.det(q)[..., None]
    return q


def random_case(seed, variant, B, N, F, C=3, D=5, Ct=4, stride=None, ignore=0.1):
    """Labels of the real kinds -- integer classes (a share `ignore` at -100), orthonormal label frames, scores in
    [0, 1] -- and predictions near them, fp32.  -> (preds, labels)"""
    rng = np.random.default_rng(seed)
    Ct = 3 if variant == CONTACT else Ct
    S = F if stride is None else stride
    f32 = np.float32
    y = rng.integers(0, C, (B, N))
    y[rng.random((B, N)) < ignore] = IGNORE
    best_R = rotations(rng, (B, F)).reshape(B, F, 9).transpose(0, 2, 1)
    R = rng.standard_normal((B, 9, N)) * 0.3
    flip = np.where(rng.random((B, 1, F)) < 0.5, NEG[None, :, None], 1.0)
    R[:, :, :F] += best_R * flip
    if variant == CURVATURE:
        best_t = rng.integers(0, Ct, (B, F))
        best_t[rng.random((B, F)) < ignore] = IGNORE
    else:
        best_t = rng.standard_normal((B, 3, F)).astype(f32)
    scene = rng.random((B, S))
    scene[rng.random((B, S)) < 0.1] = 0.0
    mov_y = (rng.random((B, D, N)) < 0.4).astype(f32)
    preds = {"score": rng.standard_normal((B, C, N)).astype(f32) * 2, "mov": rng.random((B, D, N)).astype(f32),
             "R": R.astype(f32), "t": (rng.standard_normal((B, Ct, N)) * (2.0 if variant == CURVATURE else 1.0)).astype(f32)}
    labels = {"y": y.astype(np.int64), "mov_y": mov_y, "best_R": np.ascontiguousarray(best_R).astype(f32),
              "best_t": best_t if variant == CONTACT else best_t.astype(np.int64), "scene_score": scene.astype(f32)}
    return preds, labels


# ------------------------------------------------------------------------------------------------- fixture and bounds
VARIANT_TAGS = (("curv", CURVATURE), ("cont", CONTACT))
SMOOTHING_TAGS = ("ls0", "ls1")
GRADS = (("g_score", "score"), ("g_mov", "mov"), ("g_R", "R"), ("g_t", "t"))


def load_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "loss.npz"), allow_pickle=False)


def fixture_case(g, tag, ls_tag):
    """-> (variant, preds, labels, label_smoothing, neg_weight) of one of the four recorded cases"""
    preds = {k: g["%s/pred/%s" % (tag, k)] for k in ("score", "mov", "R", "t")}
    labels = {k: g["%s/label/%s" % (tag, k)] for k in ("y", "mov_y", "best_R", "best_t", "scene_score")}
    ls = float(g["smoothings"][SMOOTHING_TAGS.index(ls_tag)])
    if ls > 0:
        labels["y"] = g[tag + "/label/y_smooth"]
    return dict(VARIANT_TAGS)[tag], preds, labels, ls, float(g["neg_weight"])


def branch_eps(g):
    """The undecided band of the two branch losses: RULE x the reference's own largest relative fp32 error on them."""
    return RULE * max(float(g[tag + "/branch_relerr"]) for tag, _ in VARIANT_TAGS)


def trace_eps(g):
    return RULE * max(float(g[tag + "/trace_abserr"]) for tag, _ in VARIANT_TAGS)


def kept_mask(preds, labels, eps):
    """(B, 9, N) bool: the frame_R gradient elements that are compared (everything but the undecided rows)."""
    B, _, N = preds["R"].shape
    keep = np.ones((B, 9, N), bool)
    und = undecided_rows(preds, labels, eps)
    keep[:, :, :und.shape[1]] &= ~und[:, None, :]
    return keep


def distances(got_losses, got_grads, want, keep):
    """Relative distance of the losses (4,) and, per gradient tensor, the largest element distance at the scale of the
    tensor's largest magnitude ({name: figure}; undecided frame_R rows left out)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        dl = np.abs(np.asarray(got_losses, np.float64) - want["losses"]) / np.abs(want["losses"])
    dg = {}
    for name, _ in GRADS:
        if got_grads.get(name) is None:
            continue
        err = np.abs(np.asarray(got_grads[name], np.float64) - want[name])
        if name == "g_R":
            err = np.where(keep, err, 0.0)
        scale = float(np.abs(want[name]).max())
        dg[name] = float(err.max()) / scale if scale > 0 else float(err.max())
    return dl, dg


def fixture_distances(g):
    """The reference's own fp32 results against the float64 yardstick: {(tag, ls_tag): (loss distances, gradient
    distances)} -- what the bounds are made of."""
    out = {}
    eps = branch_eps(g)
    for tag, _ in VARIANT_TAGS:
        for ls_tag in SMOOTHING_TAGS:
            variant, preds, labels, ls, nw = fixture_case(g, tag, ls_tag)
            want = loss(variant, preds, labels, ls, nw)
            grads = {name: g["%s/%s/grad/%s" % (tag, ls_tag, key)] for name, key in GRADS}
            out[tag, ls_tag] = distances(g["%s/%s/losses" % (tag, ls_tag)], grads, want, kept_mask(preds, labels, eps))
    return out


def bounds(g, key=None):
    """(loss bounds (4,), {gradient: bound}): RULE x the fixture's distance from float64 -- of case `key`, or the
    largest over the four cases for inputs that are not the fixture's -- with the floor LOSS_FLOOR for the losses."""
    dist = fixture_distances(g)
    keys = [key] if key is not None else sorted(dist)
    dl = np.max([dist[k][0] for k in keys], axis=0)
    dg = {name: max(dist[k][1][name] for k in keys) for name, _ in GRADS}
    return np.maximum(RULE * dl, LOSS_FLOOR), {name: RULE * v for name, v in dg.items()}


def loss_scales(variant, preds, labels, want, neg_weight=0.1):
    """What a loss's relative bound is taken of on inputs other than the fixture's.  R, t (contact) and mov are means
    of non-negative terms: the loss itself.  A cross-entropy term is the DIFFERENCE (v_y - max) - log(sum exp) in fp32:
    its error is relative to |v_y - max| and to |log(sum exp)|, not to their difference, and the sum lies in [1, K], so
    its rounding (2^-24 of the sum) passes through the logarithm as an ABSOLUTE error of that order however small the
    logarithm is -- a confident single point has a loss of 0.05 and a term error of 2^-24 all the same, in torch's fp32
    log_softmax as here.  So cls and t (curvature) take the weighted mean of |v_y - max| + |log(sum exp)| + 1 (never
    less than the loss)."""
    P, L = _f64(preds), _f64(labels)

    def ce_scale(logits, y, w, factor):
        K = logits.shape[1]
        z = logits - logits.max(axis=1, keepdims=True)
        lse = np.log(np.exp(z).sum(axis=1))
        ok = (y >= 0) & (y < K)
        yc = np.where(ok, y, 0)
        zy = np.take_along_axis(z, yc[:, None, :], axis=1)[:, 0]
        wy = np.where(ok, w[yc], 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            return factor * (wy * (np.abs(zy) + np.abs(lse) + 1.0)).sum() / wy.sum()

    scales = np.abs(np.asarray(want["losses"], np.float64)).copy()
    C = P["score"].shape[1]
    w = np.ones(C)
    w[0] = neg_weight
    scales[0] = max(scales[0], ce_scale(P["score"], L["y"], w, 1.0)) if np.isfinite(scales[0]) else scales[0]
    if variant == CURVATURE and np.isfinite(scales[2]):
        F = L["best_R"].shape[2]
        scales[2] = max(scales[2], ce_scale(P["t"][:, :, :F], L["best_t"], np.ones(P["t"].shape[1]), 0.2))
    return scales


def r_err_bound(preds, labels, want_metric, rel, eps):
    """Bound of the metric's R_err: `rel` of the value, plus what a trace that is off by `eps` moves every row's angle
    (acos is not Lipschitz at +-1: a row within eps of the clamp may move by sqrt(2 eps))."""
    c1, c2 = traces(preds, labels)
    s = _f64(labels)["scene_score"][:, :c1.shape[1]]

    def swing(c):
        return np.arccos(np.clip(c - eps, -1, 1)) - np.arccos(np.clip(c + eps, -1, 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return rel * abs(want_metric["R_err"]) + (s * np.maximum(swing(c1), swing(c2))).sum() / float(c1.size)


def clamp_rows(preds, labels, eps):
    """(B, F) bool: the rows of the metric within eps of the clamp of either branch."""
    c1, c2 = traces(preds, labels)
    return (np.abs(np.abs(c1) - 1.0) <= eps) | (np.abs(np.abs(c2) - 1.0) <= eps)
