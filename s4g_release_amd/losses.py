"""The training objective and metric of the three networks on one fused HIP call (`csrc/loss.hip`).

Mirrors of the reference's `PointNet2Loss` / `PointNet2Metric` pairs: `network_models/models/PointNet2_tcls.py:156-267`
(the curvature model, `MODEL.TYPE: "PN2_CLS"`: `PointNet2Loss`, `PointNet2Metric`) and `PointNet2.py:156-258` (the
contact model `"PN2"`, which `EdgePointNet2Down.py` builds too: `ContactPointNet2Loss`, `ContactPointNet2Metric`), with
the reference's `forward(preds, labels)` and its dictionary keys in and out.

One `s4g_grasp_loss_f32` call per `forward` gives the four losses and the unit gradient of each with respect to its own
prediction; `backward` scales those by the incoming scalars, so `sum(loss_dict.values()).backward()` and any
reweighting work.  No host synchronisation: everything runs on the current stream and can be captured in a graph, and
`loss.status` (bit 0: a score label outside [0, C) that is not -100; bit 1: the same for `best_frame_t`) is a device
tensor that the caller reads when it wants to.  INTEGRATION.md lists the decisions.  There is no CPU path.
"""
import ctypes

import torch
from torch import nn

from . import _cabi

CURVATURE, CONTACT = 0, 1
MAX_CHANNELS = 8
MAX_B = 65535
LOSS_KEYS = ("cls_loss", "R_loss", "t_loss", "mov_loss")
SCORE_KEYS = ("scene_score_logits", "score")       # the loss as written reads the first, the curvature network returns
#                                                    the second: either is accepted


def _get(d, keys, what):
    for k in keys:
        if k in d:
            return d[k]
    raise ValueError("%s has no %s" % (what, " / ".join(repr(k) for k in keys)))


def _want(t, name, dtype, shape):
    """dtype and shape of one tensor; `shape` entries of None are free."""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor (got %s)" % (name, type(t).__name__))
    if t.dtype != dtype:
        raise ValueError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if t.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
        raise ValueError("%s must have shape %s (got %s)" % (name, tuple("*" if s is None else s for s in shape),
                                                             tuple(t.shape)))


class _Inputs:
    """The validated, contiguous inputs of one call and its shapes.  Raises ValueError before anything is launched."""

    def __init__(self, variant, preds, labels):
        self.variant = variant
        score = _get(preds, SCORE_KEYS, "preds")
        mov, R, t = (_get(preds, (k,), "preds") for k in ("movable_logits", "frame_R", "frame_t"))
        y, mov_y, best_R, best_t, s = (_get(labels, (k,), "labels") for k in (
            "scene_score_labels", "scene_movable_labels", "best_frame_R", "best_frame_t", "scene_score"))
        _want(score, "score logits", torch.float32, (None, None, None))
        B, C, N = (int(v) for v in score.shape)
        _want(mov, "movable_logits", torch.float32, (B, None, N))
        D = int(mov.shape[1])
        _want(R, "frame_R", torch.float32, (B, 9, N))
        _want(t, "frame_t", torch.float32, (B, None, N))
        Ct = int(t.shape[1])
        _want(y, "scene_score_labels", torch.int64, (B, N))
        _want(mov_y, "scene_movable_labels", torch.float32, (B, D, N))
        _want(best_R, "best_frame_R", torch.float32, (B, 9, None))
        F = int(best_R.shape[2])
        if variant == CURVATURE:
            _want(best_t, "best_frame_t", torch.int64, (B, F))
        else:
            _want(best_t, "best_frame_t", torch.float32, (B, 3, F))
        _want(s, "scene_score", torch.float32, (B, None))
        if not 2 <= C <= MAX_CHANNELS:
            raise ValueError("score logits must have 2 to %d classes (got %d)" % (MAX_CHANNELS, C))
        if not 1 <= D <= MAX_CHANNELS:
            raise ValueError("movable_logits must have 1 to %d channels (got %d)" % (MAX_CHANNELS, D))
        if variant == CURVATURE and not 2 <= Ct <= MAX_CHANNELS:
            raise ValueError("frame_t must have 2 to %d classes (got %d)" % (MAX_CHANNELS, Ct))
        if variant == CONTACT and Ct != 3:
            raise ValueError("frame_t must have 3 channels (got %d)" % Ct)
        if B < 1 or N < 1 or B > MAX_B or B * N >= 2 ** 31:
            raise ValueError("needs 1 <= B <= %d, N >= 1 and B * N < 2^31 (got B = %d, N = %d)" % (MAX_B, B, N))
        if F > N:
            raise ValueError("best_frame_R has %d frame points, more than the %d points of frame_R" % (F, N))
        if int(s.shape[1]) < F:
            raise ValueError("scene_score has %d columns, fewer than the %d frame points" % (int(s.shape[1]), F))
        tensors = (score, mov, R, t, y, mov_y, best_R, best_t, s)
        for x in tensors:
            if not x.is_cuda:
                raise ValueError("the loss runs on the GPU only: every tensor must be a CUDA tensor")
        if len({x.device for x in tensors}) != 1:
            raise ValueError("every tensor must be on the same device")
        if s.stride(1) != 1 or (B > 1 and s.stride(0) < F):
            s = s.contiguous()                     # a row-sliced view keeps its stride; anything else is copied
        self.B, self.C, self.N, self.D, self.Ct, self.F = B, C, N, D, Ct, F
        self.stride = int(s.stride(0)) if B > 1 else max(F, 1)
        self.preds = tuple(x.contiguous() for x in (score, mov, R, t))
        self.labels = tuple(x.contiguous() for x in (y, mov_y, best_R, best_t)) + (s,)
        self.device = score.device

    def desc(self, weights, label_smoothing):
        d = _cabi.LossDesc()
        d.variant, d.B, d.N, d.F, d.C, d.D, d.Ct = self.variant, self.B, self.N, self.F, self.C, self.D, self.Ct
        d.scene_score_stride = self.stride
        d.label_smoothing = float(label_smoothing)
        for c, w in enumerate(weights):
            d.w[c] = float(w)
        d.score_logits, d.movable, d.frame_R, d.frame_t = (x.data_ptr() for x in self.preds)
        d.score_labels, d.movable_labels, d.best_frame_R, d.best_frame_t, d.scene_score = (
            x.data_ptr() for x in self.labels)
        nbytes = int(_cabi.lib().s4g_grasp_loss_workspace_bytes(self.B, self.N, self.F))
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        d.ws, d.ws_bytes = self.ws.data_ptr(), nbytes
        return d


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(inp, d, metric=False):
    with torch.cuda.device(inp.device):
        fn = _cabi.lib().s4g_grasp_metric_f32 if metric else _cabi.lib().s4g_grasp_loss_f32
        _cabi.check(fn(ctypes.byref(d), _stream()), "s4g_grasp_metric_f32" if metric else "s4g_grasp_loss_f32")


class _GraspLoss(torch.autograd.Function):
    """(losses (4,), status (1,) int32) of one fused call; saves the unit gradients of the predictions that need one."""

    @staticmethod
    def forward(ctx, inp, weights, label_smoothing, score, mov, R, t):
        d = inp.desc(weights, label_smoothing)
        losses = torch.empty(4, dtype=torch.float32, device=inp.device)
        status = torch.empty(1, dtype=torch.int32, device=inp.device)
        grads = [torch.empty_like(p) if need else None for p, need in zip(inp.preds, ctx.needs_input_grad[3:])]
        d.losses, d.status = losses.data_ptr(), status.data_ptr()
        d.g_score, d.g_movable, d.g_R, d.g_t = (None if g is None else g.data_ptr() for g in grads)
        _launch(inp, d)
        ctx.have = [g is not None for g in grads]
        ctx.save_for_backward(*[g for g in grads if g is not None])
        ctx.mark_non_differentiable(status)
        return losses, status

    @staticmethod
    def backward(ctx, g_losses, _g_status):
        saved = iter(ctx.saved_tensors)
        out = []
        for have, k in zip(ctx.have, (0, 3, 1, 2)):          # score <- cls, movable <- mov, frame_R <- R, frame_t <- t
            out.append(next(saved) * g_losses[k] if have else None)
        return (None, None, None) + tuple(out)


class PointNet2Loss(nn.Module):
    """The curvature model's objective (reference PointNet2_tcls.py:156-219): {"cls_loss", "R_loss", "t_loss",
    "mov_loss"} of `preds` (the network's output dictionary; the score logits under "scene_score_logits" or "score") and
    `labels` ("scene_score_labels", "scene_movable_labels", "best_frame_R", "best_frame_t", "scene_score")."""
    _VARIANT = CURVATURE

    def __init__(self, label_smoothing=0, neg_weight=0.1):
        super().__init__()
        if not 0 <= label_smoothing < 1:
            raise ValueError("label_smoothing must lie in [0, 1) (got %r)" % (label_smoothing,))
        self.label_smoothing = label_smoothing
        self.neg_weight = neg_weight
        self.status = None

    def forward(self, preds, labels):
        inp = _Inputs(self._VARIANT, preds, labels)
        weights = [self.neg_weight] + [1.0] * (inp.C - 1)
        score, mov, R, t = (_get(preds, k, "preds") for k in (SCORE_KEYS, ("movable_logits",), ("frame_R",),
                                                                ("frame_t",)))
        losses, self.status = _GraspLoss.apply(inp, weights, self.label_smoothing, score, mov, R, t)
        return dict(zip(LOSS_KEYS, losses.unbind(0)))


class ContactPointNet2Loss(PointNet2Loss):
    """The contact and edge models' objective (reference PointNet2.py:156-212): as `PointNet2Loss` with a squared
    offset error against fp32 `best_frame_t` (B, 3, F) in place of the translation classes."""
    _VARIANT = CONTACT


class PointNet2Metric(nn.Module):
    """The curvature model's metric (reference PointNet2_tcls.py:222-267): {"cls_acc" (B N,), "mov_acc" (B D N,),
    "R_err" scalar, "t_acc" (B F,)}."""
    _VARIANT = CURVATURE

    @torch.no_grad()
    def forward(self, preds, labels):
        inp = _Inputs(self._VARIANT, preds, labels)
        d = inp.desc([1.0] * inp.C, 0.0)
        dev = inp.device
        cls_acc = torch.empty(inp.B * inp.N, dtype=torch.float32, device=dev)
        mov_acc = torch.empty(inp.B * inp.D * inp.N, dtype=torch.float32, device=dev)
        t_acc = torch.empty(inp.B * inp.F, dtype=torch.float32, device=dev)
        metrics = torch.empty(2, dtype=torch.float32, device=dev)
        d.cls_acc, d.mov_acc, d.t_acc, d.metrics = (x.data_ptr() for x in (cls_acc, mov_acc, t_acc, metrics))
        _launch(inp, d, metric=True)
        out = {"cls_acc": cls_acc, "mov_acc": mov_acc, "R_err": metrics[0]}
        if self._VARIANT == CURVATURE:
            out["t_acc"] = t_acc
        else:
            out["t_err"] = metrics[1]
        return out


class ContactPointNet2Metric(PointNet2Metric):
    """The contact and edge models' metric (reference PointNet2.py:215-258): "t_err" in place of "t_acc"."""
    _VARIANT = CONTACT


# MODEL.TYPE -> (loss, metric, NEG_WEIGHT of the shipped configuration: the two yaml files say 0.5, the edge model has
# none and takes the yacs default 1.0)
LOSS_TYPES = {"PN2_CLS": (PointNet2Loss, PointNet2Metric, 0.5), "PN2": (ContactPointNet2Loss, ContactPointNet2Metric, 0.5),
              "EDGEPN2D": (ContactPointNet2Loss, ContactPointNet2Metric, 1.0)}


def build_loss(model_type, label_smoothing=0.0, neg_weight=None):
    """(loss, metric) of a `MODEL.TYPE`, as the reference's `build_pointnet2*` return beside the network; `neg_weight`
    None takes the shipped configuration's value.  Any other type raises ValueError."""
    if model_type not in LOSS_TYPES:
        raise ValueError("unsupported MODEL.TYPE %r: expected one of %s" % (model_type, sorted(LOSS_TYPES)))
    loss, metric, shipped = LOSS_TYPES[model_type]
    return loss(label_smoothing=label_smoothing, neg_weight=shipped if neg_weight is None else neg_weight), metric()
