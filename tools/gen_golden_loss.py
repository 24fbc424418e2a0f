#!/usr/bin/env python3
"""Golden fixture of the training objective and metric: the reference's OWN four classes -- `PointNet2Loss` /
`PointNet2Metric` of network_models/models/PointNet2_tcls.py (the curvature model) and of PointNet2.py (the contact
model) -- on CPU fp32 with torch autograd, on seeded inputs.  No network is needed: the classes take dictionaries.

IN-CONTAINER ONLY (imports the reference tree the way tools/gen_golden_contact.py does: over the oracle stand-in of
`pn2_ext` and a stub of `dgcnn_ext`, neither of which the loss classes call).

  tests/golden/loss.npz   B = 2, N = 515 (no multiple of 4), F = 300, C = 3, D = 5, neg_weight = 0.5 (the shipped yaml
      value), label_smoothing 0 and 0.1; per variant ("curv/", "cont/") the predictions and labels, and per smoothing
      ("ls0/", "ls1/") the four losses and the four gradients of sum(losses); the metrics once per variant.
      * score labels and (curvature) best_frame_t with some -100; the smoothed case takes `y_smooth` (the reference's
        one-hot scatter cannot take -100);
      * rows 0-19 of every scene: the zero label frame, scene_score > 0 (an exact tie L1 == L2);
      * rows 20-39 of the curvature variant: predictions whose columns 1 and 2 are zero against a full label frame --
        an exact tie too, and the one on which the two branches' gradients differ;
      * rows 40-69: scene_score == 0;  points 100-109: movable prediction == label exactly (sign(0));
      * contact-variant frame_R are true rotations (the reference's toRotMatrix of seeded 6-D logits), curvature raw.
      `*/branch_relerr`: the largest relative fp32 error of the reference's own L1 / L2 rows against float64, and
      `*/trace_abserr` of its (trace - 1) / 2: the widths of the undecided bands (tests/test_loss_ref.py).
Only arrays and names are stored.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import loss_ref as LR  # noqa: E402
from tools import gen_golden_contact as GC  # noqa: E402

B, N, F, C, D, CT = 2, 515, 300, 3, 5, 4
NEG_WEIGHT = 0.5
SMOOTHINGS = (("ls0", 0.0), ("ls1", 0.1))
SEED = 2901
PRED_KEYS = {"score": "scene_score_logits", "mov": "movable_logits", "R": "frame_R", "t": "frame_t"}
LABEL_KEYS = {"y": "scene_score_labels", "mov_y": "scene_movable_labels", "best_R": "best_frame_R",
              "best_t": "best_frame_t", "scene_score": "scene_score"}


def make_inputs(variant, seed, to_rot):
    """Seeded predictions and labels of one variant with the planted rows of the module docstring."""
    preds, labels = LR.random_case(seed, variant, B, N, F, C, D, CT, stride=F + 12)
    rng = np.random.default_rng(seed + 1)
    if variant == LR.CONTACT:                        # true rotations: the reference's toRotMatrix of noisy 6-D logits
        r6 = np.zeros((B, 6, N), np.float32)
        r6[:] = rng.standard_normal((B, 6, N))
        frame = labels["best_R"].reshape(B, 3, 3, F)                     # [b, i, j, f] = R[i][j]
        sign = np.where(rng.random((B, 1, F)) < 0.5, -1.0, 1.0)
        r6[:, :3, :F] = frame[:, :, 0, :] + 0.3 * r6[:, :3, :F]
        r6[:, 3:, :F] = frame[:, :, 1, :] * sign + 0.3 * r6[:, 3:, :F]
        preds["R"] = to_rot(torch.from_numpy(r6)).numpy().copy()
    labels["best_R"][:, :, 0:20] = 0.0               # the zero frame of invalid rows ...
    labels["scene_score"][:, 0:20] = 0.25 + 0.5 * rng.random((B, 20)).astype(np.float32)   # ... with a score
    if variant == LR.CURVATURE:
        preds["R"][:, [1, 2, 4, 5, 7, 8], 20:40] = 0.0
        labels["scene_score"][:, 20:40] = 0.25 + 0.5 * rng.random((B, 20)).astype(np.float32)
    labels["scene_score"][:, 40:70] = 0.0
    preds["mov"][:, :, 100:110] = labels["mov_y"][:, :, 100:110]
    y_smooth = labels["y"].copy()
    hole = y_smooth == LR.IGNORE
    y_smooth[hole] = rng.integers(0, C, int(hole.sum()))
    return preds, labels, y_smooth


def run_reference(loss_cls, metric_cls, preds, labels, y, smoothing):
    """The reference's classes on CPU fp32 -> (losses (4,), gradients of sum(losses), metrics)"""
    p = {PRED_KEYS[k]: torch.from_numpy(v.copy()).requires_grad_() for k, v in preds.items()}
    lab = {LABEL_KEYS[k]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in labels.items()}
    lab["scene_score_labels"] = torch.from_numpy(y.copy())
    loss = loss_cls(label_smoothing=smoothing, neg_weight=NEG_WEIGHT)(p, lab)
    sum(loss.values()).backward()
    losses = np.array([float(loss[k].detach()) for k in ("cls_loss", "R_loss", "t_loss", "mov_loss")], np.float32)
    grads = {k: p[PRED_KEYS[k]].grad.numpy().copy() for k in preds}
    with torch.no_grad():
        met = {k: v.numpy().copy() for k, v in metric_cls()(p, lab).items()}
    return losses, grads, met


def own_errors(preds, labels):
    """The reference's statements for the branch losses and the traces in fp32 against float64."""
    gt = torch.from_numpy(labels["best_R"])
    p = torch.from_numpy(preds["R"])[:, :, :F]
    L1 = ((p - gt) ** 2).mean(1, True)
    inv = gt.clone()
    for a in (1, 4, 7):
        inv[:, a:a + 2, :] = -inv[:, a:a + 2, :]
    L2 = ((p - inv) ** 2).mean(1, True)
    w1, w2 = LR.r_branches(preds, labels)
    rel = max(float(np.max(np.abs(L1[:, 0].numpy() - w1) / w1)), float(np.max(np.abs(L2[:, 0].numpy() - w2) / w2)))
    g3 = gt.transpose(1, 2).contiguous().view(B * F, 3, 3)
    g3i = g3.clone()
    g3i[:, :, 1:] = -g3i[:, :, 1:]
    p3 = p.transpose(1, 2).contiguous().view(B * F, 3, 3)
    got = []
    for g in (g3, g3i):
        M = torch.bmm(g, p3.transpose(1, 2))
        got.append(((M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2] - 1.0) / 2.0).numpy().reshape(B, F))
    c1, c2 = LR.traces(preds, labels)
    return rel, max(float(np.max(np.abs(got[0] - c1))), float(np.max(np.abs(got[1] - c2))))


def gen(out_dir):
    GC.setup()                                       # the reference tree on sys.path, over the stand-in extensions
    from grasp_proposal.network_models.functions.functions import toRotMatrix
    from grasp_proposal.network_models.models import PointNet2 as contact_mod
    from grasp_proposal.network_models.models import PointNet2_tcls as curvature_mod
    torch.set_num_threads(1)                         # one summation order, whatever the machine
    blob = {"seed": np.int64(SEED), "neg_weight": np.float64(NEG_WEIGHT),
            "smoothings": np.array([s for _, s in SMOOTHINGS], np.float64)}
    for tag, variant, mod in (("curv", LR.CURVATURE, curvature_mod), ("cont", LR.CONTACT, contact_mod)):
        preds, labels, y_smooth = make_inputs(variant, SEED + variant, toRotMatrix)
        for k, v in preds.items():
            blob["%s/pred/%s" % (tag, k)] = v
        for k, v in labels.items():
            blob["%s/label/%s" % (tag, k)] = v
        blob[tag + "/label/y_smooth"] = y_smooth
        rel, tr = own_errors(preds, labels)
        blob[tag + "/branch_relerr"], blob[tag + "/trace_abserr"] = np.float64(rel), np.float64(tr)
        for ls_tag, ls in SMOOTHINGS:
            y = labels["y"] if ls == 0.0 else y_smooth
            losses, grads, met = run_reference(mod.PointNet2Loss, mod.PointNet2Metric, preds, labels, y, ls)
            blob["%s/%s/losses" % (tag, ls_tag)] = losses
            for k, v in grads.items():
                blob["%s/%s/grad/%s" % (tag, ls_tag, k)] = v
            if ls == 0.0:
                for k, v in met.items():
                    blob["%s/metric/%s" % (tag, k)] = v
    path = os.path.join(out_dir, "loss.npz")
    np.savez_compressed(path, **blob)
    print("%s: %d bytes" % (os.path.basename(path), os.path.getsize(path)))
    return blob


def main():
    gen(os.environ.get("S4G_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden")))


if __name__ == "__main__":
    main()
