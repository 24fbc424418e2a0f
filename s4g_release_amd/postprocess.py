"""Pose decode on the device -- the step right after `PointNet2.forward` in the
reference's callers (`grasp_proposal_test.py:83` -> `utils/file_logger_cls.py`,
`grasp_detector.py:137-185`); SURVEY.md section 8f row f1.

`decode_top_poses` turns the four head tensors into the K best grasp frames per
scene entirely on the GPU, so a serving loop ships K x 18 floats per scene
instead of 21 x N.  Collision filtering (row f2) is not part of it.

Both networks decode here.  The curvature model (PN2_CLS: "score", frame_t = 4 depth-bin logits) as the reference's
callers do.  The contact model (PN2: "scene_score_logits", frame_t = the absolute grasp position (B, 3, N)) with this
project's definition: the same expected score, thresholds, order and Gram-Schmidt, and the head's absolute position
as the translation (`s4g_decode_poses_abs_f32`).  That is not a parity claim: the reference's own decode
(`GraspDetector.post_processing`, `file_logger_cls.py`) reads `predictions["score"]` and the 4-bin t decode, so with
`contact_model` it raises KeyError.
"""
import ctypes
import math
import threading
from collections import OrderedDict
from dataclasses import dataclass

import torch

from . import _cabi
from . import functions as _F

T_BINS = (0.08, 0.06, 0.04, 0.02)          # file_logger_cls.py:45, grasp_detector.py:177


def score_values(num_classes, convention="demo"):
    """`demo`: linspace(0,1,C+1)[:-1] (file_logger_cls.py:67); `detector`:
    linspace(0,1,C+1)[1:] (grasp_detector.py:147)."""
    v = torch.linspace(0, 1, num_classes + 1, dtype=torch.float64)
    return (v[:-1] if convention == "demo" else v[1:]).float()


_DEV_CONST = {}


def _dev_const(key, make, device):
    """Small constant tensors on the device, created once: a host -> device copy from pageable memory makes the HOST wait
    for everything queued in front of it on the stream (measured: a pipelined submit went from 0.6 to 10 ms of host time)."""
    k = (key, str(device))
    t = _DEV_CONST.get(k)
    if t is None:
        t = _DEV_CONST[k] = make().to(device)
    return t


_SMALL_LRU = OrderedDict()      # caller-supplied small matrices by value, at most _SMALL_LRU_MAX of them
_SMALL_LRU_MAX = 16
_SMALL_LOCK = threading.Lock()


def _small_on_device(x, dtype, device):
    """A caller's small matrix / vector (nested tuples, numpy, CPU tensor) on the device WITHOUT a per-call host -> device
    copy where the value repeats: a BOUNDED least-recently-used cache by value (16 entries -- `direction_matrix =
    camera2base[:3, :3] @ TRAIN2REAL` changes per capture on a moving camera; an unbounded cache would pin one device
    allocation per distinct pose for good).  A value holding NaN is never cached (NaN != NaN: it would miss on every
    call and leak).  A tensor that already lives on a device is passed through (`.to`): no host copy, no `.tolist()`
    synchronisation -- a serving loop that builds its matrices on the device pays nothing here."""
    if isinstance(x, torch.Tensor) and x.device.type != "cpu":
        return x.to(device=device, dtype=dtype)
    t = torch.as_tensor(x, dtype=torch.float64)
    vals = tuple(t.flatten().tolist())
    if any(v != v for v in vals):
        return t.to(dtype).to(device)
    key = (vals, tuple(t.shape), str(dtype), str(device))
    with _SMALL_LOCK:
        hit = _SMALL_LRU.get(key)
        if hit is not None:
            _SMALL_LRU.move_to_end(key)
            return hit
    d = t.to(dtype).to(device)
    with _SMALL_LOCK:
        _SMALL_LRU[key] = d
        while len(_SMALL_LRU) > _SMALL_LRU_MAX:
            _SMALL_LRU.popitem(last=False)
    return d


def expected_score(score_logits, convention="demo"):
    logits = _F._f32c(score_logits, "score")
    B, C, N = logits.shape
    vals = _dev_const(("score_values", C, convention), lambda: score_values(C, convention), logits.device)
    out = torch.empty((B, N), dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        rc = _cabi.lib().s4g_expected_score_f32(logits.data_ptr(), B, C, N, vals.data_ptr(),
                                                out.data_ptr(), _F._stream())
    _cabi.check(rc, "expected_score")
    return out


def _is_contact(predictions):
    """True for the contact model's predictions ("scene_score_logits", frame_t (B, 3, N) absolute positions)."""
    if "scene_score_logits" not in predictions:
        return False
    if predictions["frame_t"].shape[1] != 3:
        raise ValueError("contact-model predictions need frame_t of 3 channels (absolute positions), got %d"
                         % predictions["frame_t"].shape[1])
    return True


def _score_logits(predictions):
    return predictions["scene_score_logits"] if _is_contact(predictions) else predictions["score"]


def _decode(xyz, R, t, sel, contact):
    """(B, K, 4, 4) row-major poses of the points sel (B, K): `s4g_decode_poses_abs_f32` for an absolute frame_t
    (contact model), `s4g_decode_poses_f32` with the depth bins otherwise."""
    B, _, N = R.shape
    K = sel.shape[1]
    H = torch.empty((B, K, 4, 4), dtype=torch.float32, device=R.device)
    with torch.cuda.device(R.device):
        if contact:
            rc = _cabi.lib().s4g_decode_poses_abs_f32(R.data_ptr(), t.data_ptr(), sel.data_ptr(), B, N, K,
                                                      H.data_ptr(), _F._stream())
        else:
            bins = _dev_const(("t_bins", t.shape[1]), lambda: torch.tensor(T_BINS[:t.shape[1]], dtype=torch.float32),
                              R.device)
            rc = _cabi.lib().s4g_decode_poses_f32(xyz.data_ptr(), R.data_ptr(), t.data_ptr(), sel.data_ptr(), B, N,
                                                  K, t.shape[1], bins.data_ptr(), H.data_ptr(), _F._stream())
    _cabi.check(rc, "decode_poses")
    return H


def _kept_points(predictions, scene_points):
    """Predictions of `FusedPointNet2(..., topk=K)` cover a scene's K best-scoring points only and carry their point
    numbers in "index": (those points' coordinates (B, 3, K), index) -- or (scene_points, None) for a full forward."""
    idx = predictions.get("index") if hasattr(predictions, "get") else None
    if idx is None:
        return scene_points, None
    return torch.gather(scene_points, 2, idx.unsqueeze(1).expand(-1, 3, -1)).contiguous(), idx


def decode_top_poses(predictions, scene_points, num_poses=50, convention="demo"):
    """-> (H (B,K,4,4) fp32, score (B,K) fp32, index (B,K) int64), best first
    (file_logger_cls.py:196-218: K = 50, argsort(-score)[:K], Gram-Schmidt).  Predictions over a scene's kept points
    (`FusedPointNet2(..., topk=)`) are accepted too: the returned index numbers the scene's points either way.
    Contact-model predictions take frame_t as the translation (module docstring)."""
    scene_points, kept = _kept_points(predictions, scene_points)
    if kept is not None:
        H, top, sel = decode_top_poses({k: v for k, v in predictions.items() if k != "index"}, scene_points,
                                       num_poses, convention)
        return H, top, torch.gather(kept, 1, sel)
    xyz = _F._f32c(scene_points, "scene_points")
    R = _F._f32c(predictions["frame_R"], "frame_R")
    t = _F._f32c(predictions["frame_t"], "frame_t")
    score = expected_score(_score_logits(predictions), convention)
    B, _, N = xyz.shape
    K = min(int(num_poses), N)
    top, sel = torch.topk(score, K, dim=1, largest=True, sorted=True)
    sel = sel.contiguous()
    return _decode(xyz, R, t, sel, _is_contact(predictions)), top, sel


REAL2TRAIN = ((0., 1., 0., 0.), (1., 0., 0., 0.), (0., 0., -1., 0.), (0., 0., 0., 1.))   # grasp_detector.py:26
TRAIN2REAL = REAL2TRAIN                               # :27 (the matrix is its own inverse)


def _detect_poses_as_written(predictions, scene_points, score_threshold, verticalness_threshold,
                             direction_matrix, vertical_direction, frame, max_poses):
    """`GraspDetector.post_processing` with the reference's indexing EXACTLY as written
    (grasp_detector.py:149-167), on the device.  Two quirks of those lines are reproduced:
      * :150-153 `index_high2low` (positions inside `high_score_index`, best score first) indexes
        the POINT axis of `frame_R`;
      * :154 `rotation.transpose(0, 1)` is a numpy call, i.e. the identity permutation, so the
        (9, n) array is reshaped row-major into n 3x3 blocks: block m, entry e is the flat element
        f = 9 m + e of the (9, n) array = frame_R[f // n, index_high2low[f % n]].
    Block m is then paired with point high_score_index[m] (:160-167); survivors of the verticalness
    test keep ASCENDING point order.  The expected score is formed like the reference's (fp32
    softmax, float64 weighted sum) so that thresholding and ordering see the same numbers."""
    xyz = _F._f32c(scene_points, "scene_points")
    B, _, N = xyz.shape
    dev = xyz.device
    K = min(int(max_poses), N)
    dm = torch.eye(3, dtype=torch.float64, device=dev) if direction_matrix is None else \
        torch.as_tensor(direction_matrix, dtype=torch.float64, device=dev)
    v = torch.as_tensor(vertical_direction, dtype=torch.float32, device=dev).double()
    vals = torch.linspace(0, 1, predictions["score"].shape[1] + 1, dtype=torch.float64, device=dev)[1:]
    bins = torch.tensor(T_BINS[:predictions["frame_t"].shape[1]], dtype=torch.float32, device=dev)
    fr = torch.as_tensor(frame, dtype=torch.float32, device=dev)
    H = torch.zeros((B, K, 4, 4), dtype=torch.float32, device=dev)
    top = torch.zeros((B, K), dtype=torch.float32, device=dev)
    sel = torch.full((B, K), -1, dtype=torch.int64, device=dev)
    count = torch.zeros((B,), dtype=torch.int64, device=dev)
    for b in range(B):       # ragged per scene (the reference itself only accepts B == 1, :49)
        prob = torch.softmax(predictions["score"][b].float(), dim=0)                  # :143
        score = (vals.view(-1, 1) * prob.double()).sum(dim=0)                          # :145-146
        high = torch.nonzero(score > score_threshold).flatten()                        # :149
        n = int(high.numel())
        if n == 0:
            continue
        h2l = torch.argsort(score[high], descending=True)                              # :150
        flat = predictions["frame_R"][b].float()[:, h2l].reshape(-1)                   # :153, (9 n,)
        rot = flat.view(n, 3, 3)                                                       # :154
        xdir = -(dm @ rot[:, :, 0].double().t())                                       # :155, (3, n)
        vertical = (xdir.t() * v.view(1, 3)).sum(dim=1)                                # :156
        good = torch.nonzero(vertical > verticalness_threshold).flatten()              # :157
        valid = high[good][:K]                                                         # :160
        good = good[:K]
        m = int(valid.numel())
        if m == 0:
            continue
        # the decode kernel works on (9, m) / (tc, m) / (3, m) columns: hand it the blocks as columns
        Rm = rot[good].reshape(m, 9).t().contiguous().unsqueeze(0)                     # :164
        tm = predictions["frame_t"][b].float()[:, valid].contiguous().unsqueeze(0)     # :165
        pm = xyz[b][:, valid].contiguous().unsqueeze(0)                                # :163
        ar = torch.arange(m, dtype=torch.int64, device=dev).unsqueeze(0)
        Hb = torch.empty((1, m, 4, 4), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _cabi.lib().s4g_decode_poses_f32(pm.data_ptr(), Rm.data_ptr(), tm.data_ptr(),
                                                  ar.data_ptr(), 1, m, m, tm.shape[1], bins.data_ptr(),
                                                  Hb.data_ptr(), _F._stream())
        _cabi.check(rc, "decode_poses")
        H[b, :m] = torch.matmul(fr.view(1, 4, 4), Hb[0])                               # :180
        top[b, :m] = score[valid].float()                                              # :167
        sel[b, :m] = valid
        count[b] = m
    return H, top, sel, count


def detect_poses(predictions, scene_points, score_threshold=0.7, verticalness_threshold=0.2,
                 direction_matrix=None, vertical_direction=(0.0, 0.0, 1.0), frame=TRAIN2REAL,
                 max_poses=1024, reference_indexing=False):
    """`GraspDetector.post_processing` (grasp_detector.py:137-185) for a whole batch, on the device
    and without a host round trip: expected score with the detector's class values (:145-146),
    score threshold (:149), survivors in descending score order (:150-151), verticalness filter
    `(-direction_matrix @ R[:, 0]) . vertical_direction > threshold` (:155-157; direction_matrix is
    the caller's `camera2base[:3,:3] @ TRAIN2REAL[:3,:3]`, identity if None), translation decode
    and Gram-Schmidt (:124-135,177-179), result moved into the caller's frame (`frame @ H`, :180).

    Returns (H (B, max_poses, 4, 4) fp32, score (B, max_poses), index (B, max_poses) int64,
    count (B,) int64): per scene the first count[b] rows are the detections, best first; rows past
    the count are zero / -1.

    Default: every pose is built from its OWN point's rotation and translation, best score first --
    what the reference's comments describe.  `reference_indexing=True` reproduces what its lines
    :149-167 actually compute (a position list used as point indices and a numpy transpose that is
    a no-op; see `_detect_poses_as_written`): same poses, scores and order as the reference, pinned
    by tests/golden/post_detector.npz which the reference's own function generated.

    Contact-model predictions ("scene_score_logits", frame_t (B, 3, N) absolute grasp positions) take the same
    expected score, thresholds, order, verticalness on R[:, :, 0] and `frame @ H`, with the head's absolute position
    as the translation (`s4g_decode_poses_abs_f32`).  This is this project's definition, not a reference parity
    claim: the reference's own `post_processing` reads `predictions["score"]` and decodes t from 4 depth bins, so
    with `contact_model` it raises KeyError.  `reference_indexing=True` raises ValueError for them."""
    contact = _is_contact(predictions)
    if contact and reference_indexing:
        raise ValueError("reference_indexing=True restates the reference's curvature-model post_processing: it does not "
                         "apply to contact-model predictions")
    scene_points, kept = _kept_points(predictions, scene_points)
    if kept is not None:
        # (exact whenever the kept points contain every candidate the filters would pass among the best max_poses:
        #  always when fewer than K points of a scene exceed the score threshold)
        if reference_indexing:
            raise ValueError("reference_indexing=True restates the reference's point-axis quirks: it needs the full forward")
        H, top, sel, count = detect_poses({k: v for k, v in predictions.items() if k != "index"}, scene_points,
                                          score_threshold, verticalness_threshold, direction_matrix=direction_matrix,
                                          vertical_direction=vertical_direction, frame=frame, max_poses=max_poses)
        return H, top, torch.where(sel >= 0, torch.gather(kept, 1, sel.clamp(min=0)), sel), count
    if reference_indexing:
        return _detect_poses_as_written(predictions, scene_points, score_threshold, verticalness_threshold,
                                        direction_matrix, vertical_direction, frame, max_poses)
    xyz = _F._f32c(scene_points, "scene_points")
    R = _F._f32c(predictions["frame_R"], "frame_R")
    t = _F._f32c(predictions["frame_t"], "frame_t")
    score = expected_score(_score_logits(predictions), "detector")              # (B, N)
    B, _, N = xyz.shape
    dev = xyz.device
    dm = _small_on_device(((1., 0., 0.), (0., 1., 0.), (0., 0., 1.)) if direction_matrix is None else direction_matrix,
                          torch.float32, dev)
    v = _small_on_device(vertical_direction, torch.float32, dev)
    w = -(dm.t() @ v)                                                           # (-A r0) . v == r0 . (-A^T v)
    r0 = R.view(B, 3, 3, N)[:, :, 0, :]                                         # first column of every R
    vertical = (r0 * w.view(1, 3, 1)).sum(dim=1)                                # (B, N)
    keep = (score > score_threshold) & (vertical > verticalness_threshold)
    key = torch.where(keep, score, torch.full_like(score, float("-inf")))
    K = min(int(max_poses), N)
    top, sel = torch.sort(key, dim=1, descending=True, stable=True)
    top, sel = top[:, :K], sel[:, :K].contiguous()
    count = keep.sum(dim=1).clamp(max=K)
    H = _decode(xyz, R, t, sel, contact)
    fr = _small_on_device(frame, torch.float32, dev)
    # frame @ H for every pose: a broadcast multiply + sum over the 4-long contraction (one elementwise kernel + one
    # reduction) -- `torch.matmul` dispatches 32 768 4x4 products to a batched library GEMM: 0.52 ms per call in the
    # detect loop's kernel trace (profiles/r06_detect_kernel_stats.md)
    H = (fr.view(1, 1, 4, 4, 1) * H.unsqueeze(2)).sum(dim=3)
    valid = torch.arange(K, device=dev).view(1, K) < count.view(B, 1)
    H = torch.where(valid.view(B, K, 1, 1), H, torch.zeros_like(H))
    top = torch.where(valid, top, torch.zeros_like(top))
    sel = torch.where(valid, sel, torch.full_like(sel, -1))
    return H, top, sel, count


def importance_sampling(score, count, num_selected, generator=None, uniforms=None):
    """grasp_detector.py:237-251 on the device: `num_selected` draws per scene from the first
    count[b] poses with probability proportional to exp(5 score) (sorted uniforms against the
    cumulative sum = systematic inverse-CDF sampling).  Returns indices (B, num_selected) into the
    pose list (ascending); scenes with count <= num_selected keep 0..count-1 (padded with -1)."""
    B, K = score.shape
    dev = score.device
    valid = torch.arange(K, device=dev).view(1, K) < count.view(B, 1)
    wgt = torch.where(valid, torch.exp(5.0 * score.double()), torch.zeros((), dtype=torch.float64, device=dev))
    cum = torch.cumsum(wgt, dim=1)
    if uniforms is not None:      # the draws passed in (tests; the reference calls np.random.rand(num_selected) unseeded)
        u = torch.as_tensor(uniforms, dtype=torch.float64).to(dev).reshape(-1, num_selected).expand(B, -1)
    else:
        u = torch.rand((B, num_selected), generator=generator, device=dev, dtype=torch.float64)
    target = torch.sort(u, dim=1)[0] * cum[:, -1:]
    pick = torch.searchsorted(cum, target, right=False).clamp(max=K - 1)
    ar = torch.arange(num_selected, device=dev).view(1, -1).expand(B, -1)
    few = count.view(B, 1) <= num_selected
    pick = torch.where(few, torch.where(ar < count.view(B, 1), ar, torch.full_like(ar, -1)), pick)
    return pick


@dataclass
class GripperConfig:
    """configs/gripper_config.py:10-21 and processing_config.py:25,37-40."""
    half_bottom_width: float = 0.057
    bottom_length: float = 0.16
    finger_width: float = 0.023
    half_hand_thickness: float = 0.012
    finger_length: float = 0.09
    back_collision_margin: float = 0.0
    back_collision_threshold: float = 10 * math.sqrt(8)
    finger_collision_threshold: float = 10
    close_region_min_points: float = 50         # eval_experiment/config.py:43
    neighbor_depth: float = 0.005               # eval_experiment/config.py:48

    @property
    def half_bottom_space(self):
        return self.half_bottom_width - self.finger_width


def se3_inverse(poses):
    """`torch_batch_transformation_inv` (utils/math_utils.py:26-40) for (..., 4, 4) fp32 poses:
    [R^T | -R^T t], the form `GraspDetector.detect` feeds the collision check (grasp_detector.py:219)."""
    T = poses.float()
    Rt = T[..., :3, :3].transpose(-1, -2)
    out = torch.zeros_like(T)
    out[..., :3, :3] = Rt
    out[..., :3, 3:] = torch.matmul(-Rt, T[..., :3, 3:])
    out[..., 3, 3] = 1.0
    return out.contiguous()


_ABSENT = object()     # (an entry point without scene normals; None is a caller's value and is checked like any other)


def _dense_scene(scene_points, scene_labels, scene_normals=_ABSENT, same_device=(), size="N", nonempty=False):
    """The dense scene the frame-grading entry points share, checked in one place: scene_points (B, 3, size) fp32,
    scene_labels (B, size) int32 and, where the entry point takes them, scene_normals like the points, all on the
    device of `same_device`, the (name, CUDA tensor) pairs the message names first.
    -> (xyz, nrm or None, lab, B, size, device), contiguous.  The checks run in this order, before the caller's own
    checks of its other tensors: a call that is wrong in two arguments may name the other one first."""
    xyz = _F._f32c(scene_points, "scene_points")
    nrm = None if scene_normals is _ABSENT else _F._f32c(scene_normals, "scene_normals")
    if not isinstance(scene_labels, torch.Tensor) or scene_labels.device.type != "cuda":
        raise RuntimeError("scene_labels must be a CUDA tensor (there is no CPU fallback)")
    if scene_labels.dtype != torch.int32:
        raise RuntimeError("scene_labels must be int32, got %s" % scene_labels.dtype)
    if xyz.dim() != 3 or xyz.size(1) != 3 or (nonempty and xyz.size(2) < 1):
        raise RuntimeError("scene_points must be (B, 3, %s)" % size)
    B, _, N = xyz.shape
    if nrm is not None and tuple(nrm.shape) != (B, 3, N):
        raise RuntimeError("scene_normals must be (B, 3, %s) like scene_points" % size)
    if tuple(scene_labels.shape) != (B, N):
        raise RuntimeError("scene_labels must be (B, %s)" % size)
    named = list(same_device) + [("scene_points", xyz)] + ([] if nrm is None else [("scene_normals", nrm)]) + \
        [("scene_labels", scene_labels)]
    if len({t.device for _, t in named}) != 1:
        names = [n for n, _ in named]
        raise RuntimeError("%s and %s must live on one device" % (", ".join(names[:-1]), names[-1]))
    return xyz, nrm, scene_labels.contiguous(), B, N, xyz.device


def _scene_count(count, B, device, name):
    """The optional per-scene row count `name` (B,) -> int64 on the device, or None."""
    if count is None:
        return None
    if tuple(count.shape) != (B,):
        raise RuntimeError("%s must be (B,)" % name)
    return count.to(device=device, dtype=torch.int64).contiguous()


def _g2l_of(poses, inverse):
    """`inverse=` of the pose entry points -> (the matrices the kernel reads, its invert_se3 flag).  "se3": the poses
    themselves, the kernel forms [R^T | -R^T t] (one launch; a batched library GEMM of 3x3 blocks took 0.26 ms);
    "general": their float64 inverse rounded to fp32."""
    if inverse not in ("general", "se3"):
        raise ValueError("inverse must be 'general' or 'se3'")
    if inverse == "se3":
        return poses.float().contiguous(), 1
    return torch.linalg.inv(poses.double()).float().contiguous(), 0


def _workspace(nbytes, device):
    """What a `*_workspace_bytes` call returned -> (uint8 tensor of that many bytes, at least one; the byte count as int):
    the two workspace arguments of the entry point."""
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device), int(nbytes)


def view_non_collision(poses, scene_points, gripper=None, inverse="general", count=None):
    """Batched `CloudCollisionChecker.view_non_collision`
    (cloud_processor/view_collision_checker.py:37-65) for all poses of all scenes
    in one launch.  poses (B,K,4,4) gripper->global frames; returns
    (ok (B,K) bool, counts (B,K,2) int32).  inverse="general": the inverse is taken in float64 and
    rounded to fp32 like the demo's caller (file_logger_cls.py:223-224); inverse="se3": the fp32
    analytic SE(3) inverse the detector uses (grasp_detector.py:219, `se3_inverse`).
    count (B,) int64 on the device (optional): only the first count[b] rows of scene b are poses (the padded best-first
    lists of `detect_poses`); the other rows are not scanned, read ok = False and zero counts."""
    gripper = gripper or GripperConfig()
    xyz = _F._f32c(scene_points, "scene_points")
    B, _, N = xyz.shape
    K = poses.shape[1]
    g2l, invert = _g2l_of(poses, inverse)
    counts = torch.empty((B, K, 2), dtype=torch.int32, device=xyz.device)
    params = (ctypes.c_float * 6)(gripper.finger_length, gripper.bottom_length,
                                  gripper.half_hand_thickness, gripper.half_bottom_width,
                                  gripper.half_bottom_space, gripper.back_collision_margin)
    with torch.cuda.device(xyz.device):
        if count is None and not invert:
            rc = _cabi.lib().s4g_collision_counts_f32(xyz.data_ptr(), g2l.data_ptr(), B, N, K, params,
                                                      counts.data_ptr(), _F._stream())
        else:
            # (not `_scene_count`, nor `_dense_scene` above: this entry point has never checked these shapes)
            cnt = None if count is None else count.to(device=xyz.device, dtype=torch.int64).contiguous()
            rc = _cabi.lib().s4g_collision_counts_n_f32(xyz.data_ptr(), g2l.data_ptr(), B, N, K, params,
                                                        None if cnt is None else cnt.data_ptr(), invert,
                                                        counts.data_ptr(), _F._stream())
    _cabi.check(rc, "collision_counts")
    ok = (counts[..., 0] <= gripper.back_collision_threshold) & \
         (counts[..., 1] <= gripper.finger_collision_threshold)
    if count is not None:
        ok = ok & (torch.arange(K, device=xyz.device).view(1, K) < count.view(B, 1))
    return ok, counts


@dataclass
class FrameEvaluation:
    """What `eval_frames` returns: (B, K) device tensors, one entry per pose row.  `back`, `finger`, `close`, `n_left`,
    `n_right` int32; `collision`, `multi_objects` bool; `left_y`, `right_y`, `mean_left`, `mean_right`, `score` fp32.
    `ints` (B, K, 8) and `floats` (B, K, 5) are the kernel's own output tensors (include/s4g_ops.h has the layout);
    the named fields are views of them."""
    ints: torch.Tensor
    floats: torch.Tensor

    back = property(lambda self: self.ints[..., 0])
    finger = property(lambda self: self.ints[..., 1])
    close = property(lambda self: self.ints[..., 2])
    multi_objects = property(lambda self: self.ints[..., 3] != 0)
    n_left = property(lambda self: self.ints[..., 4])
    n_right = property(lambda self: self.ints[..., 5])
    collision = property(lambda self: self.ints[..., 6] != 0)
    left_y = property(lambda self: self.floats[..., 0])
    right_y = property(lambda self: self.floats[..., 1])
    mean_left = property(lambda self: self.floats[..., 2])
    mean_right = property(lambda self: self.floats[..., 3])
    score = property(lambda self: self.floats[..., 4])


def eval_frames(poses, scene_points, scene_normals, scene_labels, gripper=None, inverse="general", count=None):
    """Batched `EvalExpCloud.eval_frame` (eval_experiment/eval_point_cloud.py:39-113): every pose of every scene graded
    against the scene's dense labelled cloud in one sync-free call -> `FrameEvaluation`.

    poses (B, K, 4, 4) gripper -> global frames; scene_points, scene_normals (B, 3, N) fp32; scene_labels (B, N)
    int32.  `inverse=` and `count=` as in `view_non_collision` (rows at or past count[b] are not scanned and read
    zero / False everywhere).  Per pose: the counts behind the palm and in the fingers (equal to `view_non_collision`'s
    bit for bit), the number of points in the close region, `collision`, `multi_objects` (more than one label in the
    close region) and, when the region holds at least `gripper.close_region_min_points` points and neither flag is
    set, the antipodal score mean |n.y| under the left pad times the same under the right pad; else score 0.
    Normals and labels are inputs, as for the reference, which reads them from a file: normal estimation (open3d),
    the baseline variant eval_point_cloud_baseline.py and data_gen/ are out of scope."""
    gripper = gripper or GripperConfig()
    if not isinstance(poses, torch.Tensor) or poses.device.type != "cuda":
        raise RuntimeError("poses must be a CUDA tensor (there is no CPU fallback)")
    xyz, nrm, lab, B, N, dev = _dense_scene(scene_points, scene_labels, scene_normals, [("poses", poses)])
    if poses.dim() != 4 or poses.size(0) != B or tuple(poses.shape[2:]) != (4, 4):
        raise RuntimeError("poses must be (B, K, 4, 4)")
    g2l, invert = _g2l_of(poses, inverse)
    K = poses.shape[1]
    cnt = _scene_count(count, B, dev, "count")
    ints = torch.empty((B, K, 8), dtype=torch.int32, device=dev)
    floats = torch.empty((B, K, 5), dtype=torch.float32, device=dev)
    params = (ctypes.c_float * 10)(gripper.finger_length, gripper.bottom_length, gripper.half_hand_thickness,
                                   gripper.half_bottom_width, gripper.half_bottom_space, gripper.back_collision_margin,
                                   gripper.back_collision_threshold, gripper.finger_collision_threshold,
                                   gripper.close_region_min_points, gripper.neighbor_depth)
    ws, nbytes = _workspace(_cabi.lib().s4g_eval_frames_workspace_bytes(B, N, K), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_eval_frames_f32(xyz.data_ptr(), nrm.data_ptr(), lab.data_ptr(), g2l.data_ptr(), B, N, K,
                                             params, None if cnt is None else cnt.data_ptr(), invert,
                                             ints.data_ptr(), floats.data_ptr(), ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "eval_frames")
    return FrameEvaluation(ints, floats)


LS_MAX_DEPTHS, LS_MAX_ANGLES = 8, 16        # the compiled maxima of csrc/local_search.hip


@dataclass
class LocalSearchConfig:
    """The constants of the data generator's local search (data_gen/configs/config.py:17-56,89) and the label of a
    placement without one (`len(NAME_LIST)`, torch_single_view_point_cloud.py:74-75)."""
    table_height: float = 0.75
    num_points_threshold: float = 8
    length_search: tuple = (-0.08, -0.06, -0.04, -0.02)
    thickness_search: tuple = (0,)
    theta_search_deg: tuple = tuple(range(-90, 90, 15))
    back_collision_threshold: float = 0 * math.sqrt(8)
    back_collision_margin: float = 0.0
    finger_collision_threshold: float = 0
    close_region_min_points: float = 10
    neighbor_depth: float = 0.005
    half_bottom_width: float = 0.057
    bottom_length: float = 0.08
    finger_width: float = 0.023
    half_hand_thickness: float = 0.012
    finger_length: float = 0.09
    table_collision_offset: float = 0.005
    no_label: int = 122

    @property
    def half_bottom_space(self):
        return self.half_bottom_width - self.finger_width

    @property
    def shape(self):
        """(L, T): depths and roll angles per depth (GRASP_PER_LENGTH)."""
        return len(self.length_search), len(self.theta_search_deg) * len(self.thickness_search)

    def check(self):
        if len(self.thickness_search) != 1 or float(self.thickness_search[0]) != 0.0:
            raise ValueError("THICKNESS_SEARCH must stay [0], the only value the reference ships: a non-zero height "
                             "is not implemented")
        L, T = self.shape
        if not (1 <= L <= LS_MAX_DEPTHS and 1 <= T <= LS_MAX_ANGLES):
            raise ValueError("need 1..%d depths and 1..%d angles, got %d and %d" % (LS_MAX_DEPTHS, LS_MAX_ANGLES, L, T))

    def tables(self):
        """The fp32 values the reference works with, formed as it forms them: theta = deg / 57.29578 in Python floats
        (config.py:44), rows (length, theta, height) to one fp32 tensor (:74), torch.cos / torch.sin of its theta
        column (:79-82).  -> dict of fp32 CPU tensors `depth` (L), `cos`, `sin` (T), and the slab bounds `lo`, `hi` (L)
        = dl - BOTTOM_LENGTH, dl + FINGER_LENGTH in Python floats, rounded once (:270-271)."""
        self.check()
        rows = [(float(length), deg / 57.29578, float(h)) for length in self.length_search
                for deg in self.theta_search_deg for h in self.thickness_search]
        a = torch.tensor(rows)
        L, T = self.shape
        cos, sin = torch.cos(a[:, 1])[:T].clone(), torch.sin(a[:, 1])[:T].clone()
        return {"depth": a[::T, 0].clone(), "cos": cos, "sin": sin,
                "lo": torch.tensor([float(v) - self.bottom_length for v in self.length_search]),
                "hi": torch.tensor([float(v) + self.finger_length for v in self.length_search])}

    def search_to_local(self):
        """LOCAL_SEARCH_TO_LOCAL (config.py:88) as (L, T, 4, 4) fp32, formed directly instead of by `torch.inverse`: the
        inverse roll and the shift dl along x."""
        tb = self.tables()
        L, T = self.shape
        S = torch.zeros(L, T, 4, 4)
        S[..., 0, 0] = S[..., 3, 3] = 1.0
        S[..., 0, 3] = tb["depth"].view(L, 1)
        S[..., 1, 1] = S[..., 2, 2] = tb["cos"].view(1, T)
        S[..., 1, 2] = -tb["sin"].view(1, T)
        S[..., 2, 1] = tb["sin"].view(1, T)
        return S


@dataclass
class LocalSearch:
    """What `grade_local_search` returns: device tensors, one row per frame.  `ints` (B, F, L, T, 6), `scores`
    (B, F, L, T), `slab_count` (B, F, L), `valid_index` (B, F) and `count` (B,) are the kernel's own outputs
    (include/s4g_ops.h has the layout); the named fields are views of them."""
    ints: torch.Tensor
    scores: torch.Tensor
    slab_count: torch.Tensor
    valid_i32: torch.Tensor
    valid_index: torch.Tensor
    count: torch.Tensor
    points: torch.Tensor
    frames: torch.Tensor
    config: LocalSearchConfig
    unbatched: bool = False

    search_score = property(lambda self: self.ints[..., 0])
    objects_label = property(lambda self: self.ints[..., 1])
    back = property(lambda self: self.ints[..., 2])
    finger = property(lambda self: self.ints[..., 3])
    close = property(lambda self: self.ints[..., 4])
    table_collision = property(lambda self: self.ints[..., 5] != 0)
    antipodal_score = property(lambda self: self.scores)
    valid = property(lambda self: self.valid_i32 != 0)

    def frames_of(self, index=None):
        """The reference's `valid_frame` (:351-356) of the frames `index` (B, M) (default: `valid_index`): (B, M, L, T,
        4, 4) = [R | p] @ LOCAL_SEARCH_TO_LOCAL, formed directly (no `torch.inverse`).  Rows whose index is -1 are 0."""
        index = self.valid_index if index is None else index
        idx = index.to(device=self.points.device, dtype=torch.int64)
        B, F = self.points.shape[:2]
        M = idx.shape[1]
        live = (idx >= 0).view(B, M, 1, 1, 1, 1)
        g = idx.clamp(min=0)
        H = torch.zeros((B, M, 4, 4), dtype=torch.float32, device=self.points.device)
        H[..., :3, :3] = torch.gather(self.frames, 1, g.view(B, M, 1, 1).expand(B, M, 3, 3))
        H[..., :3, 3] = torch.gather(self.points, 1, g.view(B, M, 1).expand(B, M, 3))
        H[..., 3, 3] = 1.0
        S = _small_on_device(self.config.search_to_local(), torch.float32, self.points.device)
        return torch.where(live, torch.matmul(H.view(B, M, 1, 1, 4, 4), S), torch.zeros((), device=H.device))

    def dump(self, b=0):
        """The dictionary of the reference's `dump()` (:203-222) for scene b, in the world frame (the camera transform is
        the caller's); `point_cloud` holds the frame origins (3, F).  Reads the count on the host."""
        n = int(self.count[b])
        vi = self.valid_index[b, :n].long()
        return {"search_score": self.search_score[b, vi].cpu().numpy(),
                "antipodal_score": self.antipodal_score[b, vi].cpu().numpy(),
                "objects_label": self.objects_label[b, vi].to(torch.int16).cpu().numpy(),
                "point_cloud": self.points[b].t().contiguous().cpu().numpy(),
                "valid_index": vi.int().cpu().numpy(),
                "valid_frame": self.frames_of(self.valid_index[b:b + 1, :n])[0].cpu().numpy()
                if n else torch.zeros((0,) + self.config.shape + (4, 4)).numpy()}


def grade_local_search(points, frames, scene_points, scene_normals, scene_labels, config=None, frame_count=None):
    """The data generator's per-point local grasp search -- `TorchSingleViewPointCloud.finger_hand` with
    `_table_collision_check` and `_antipodal_score` (data_gen/pcd_classes/torch_single_view_point_cloud.py:152-180,
    224-358), which `run_score` (:198-201) loops over the frames -- for every frame of every scene in one sync-free,
    graph-capturable call -> `LocalSearch`.

    points (B, F, 3) frame origins and frames (B, F, 3, 3) with the x, y, z axes as columns (`self.frame`; frame
    estimation is out of scope, as for `TorchPrecomputedSingleViewPointCloud`); scene_points, scene_normals (B, 3, N)
    fp32; scene_labels (B, N) int32; unbatched inputs get a leading 1.  frame_count (B,) on the device (optional): only
    the first frame_count[b] rows of scene b are frames, the others are not scanned and read as invalid.  Per frame,
    L x T placements (4 depths x 12 rolls as shipped): `search_score`, `objects_label`, `antipodal_score`,
    `table_collision`, the counts `back` / `finger` / `close` behind every verdict (0 where the table gate skips), `slab_count` per depth, `valid`,
    and per scene the ascending `valid_index` (padded with -1) and `count`.

    Three decisions differ from running the reference as written.  (1) No stale slots: the reference writes a frame's
    results into slot `valid_grasp` and does not clear it when the frame is rejected, so they leak into the next
    accepted frame wherever that one skips a placement; here every frame's row holds its own results only.  (2) A
    close region whose points all share one y gives empty bands: the score is NaN, as `eval_frames` gives (the frame
    then counts as valid, as `torch.max` of a NaN does in the reference).  (3) `valid_frame` is formed directly
    (`LocalSearch.frames_of`), without `torch.inverse`; THICKNESS_SEARCH stays [0]."""
    cfg = config or LocalSearchConfig()
    cfg.check()
    for name, t in (("points", points), ("frames", frames), ("scene_labels", scene_labels)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    unbatched = points.dim() == 2
    if unbatched:
        points, frames = points[None], frames[None]
        scene_points, scene_normals, scene_labels = scene_points[None], scene_normals[None], scene_labels[None]
    xyz, nrm, lab, B, N, dev = _dense_scene(scene_points, scene_labels, scene_normals,
                                            [("points", points), ("frames", frames)])
    if points.dtype != torch.float32 or frames.dtype != torch.float32:
        raise RuntimeError("points and frames must be float32")
    if points.dim() != 3 or points.size(0) != B or points.size(2) != 3:
        raise RuntimeError("points must be (B, F, 3)")
    F = points.shape[1]
    if tuple(frames.shape) != (B, F, 3, 3):
        raise RuntimeError("frames must be (B, F, 3, 3)")
    pts, frm = points.contiguous(), frames.contiguous()
    cnt = _scene_count(frame_count, B, dev, "frame_count")
    L, T = cfg.shape
    tb = cfg.tables()
    tables = _small_on_device(torch.cat([tb["depth"], tb["lo"], tb["hi"], tb["cos"], tb["sin"]]), torch.float32, dev)
    ints = torch.empty((B, F, L, T, 6), dtype=torch.int32, device=dev)
    scores = torch.empty((B, F, L, T), dtype=torch.float32, device=dev)
    slab = torch.empty((B, F, L), dtype=torch.int32, device=dev)
    valid = torch.empty((B, F), dtype=torch.int32, device=dev)
    valid_index = torch.empty((B, F), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int64, device=dev)
    params = (ctypes.c_float * 13)(cfg.finger_length, cfg.bottom_length, cfg.half_hand_thickness, cfg.half_bottom_width,
                                   cfg.half_bottom_space, cfg.back_collision_margin, cfg.back_collision_threshold,
                                   cfg.finger_collision_threshold, cfg.close_region_min_points, cfg.neighbor_depth,
                                   cfg.table_height, cfg.table_height + cfg.table_collision_offset,
                                   cfg.num_points_threshold)
    ws, nbytes = _workspace(_cabi.lib().s4g_local_search_workspace_bytes(B, N, F, L, T), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_local_search_f32(pts.data_ptr(), frm.data_ptr(), xyz.data_ptr(), nrm.data_ptr(),
                                              lab.data_ptr(), B, N, F, L, T, params, int(cfg.no_label),
                                              tables.data_ptr(), None if cnt is None else cnt.data_ptr(),
                                              ints.data_ptr(), scores.data_ptr(), slab.data_ptr(), valid.data_ptr(),
                                              valid_index.data_ptr(), count.data_ptr(), ws.data_ptr(), nbytes,
                                              _F._stream())
    _cabi.check(rc, "local_search")
    return LocalSearch(ints, scores, slab, valid, valid_index, count, pts, frm, cfg, unbatched)


CURVATURE_RADIUS = 0.01                    # data_gen/configs/config.py:37
SAMPLE_REGION_OFFSET = 0.015               # SAMPLE_REGION = TABLE_HEIGHT + 0.015 (config.py:18)


@dataclass
class DarbouxFrames:
    """What `estimate_frames` returns: device tensors, one row per frame.  `frames` (B, F, 3, 3) with the axes as
    columns, `points` (B, F, 3), `count` (B, F) the neighbour count, `flags` (B, F) the kernel's own (bit 0 =
    estimated, bit 1 = degenerate), `frame_index` (B, F) int32 padded with -1 and `frame_count` (B,) int64 or None."""
    frames: torch.Tensor
    points: torch.Tensor
    count: torch.Tensor
    flags: torch.Tensor
    frame_index: torch.Tensor
    frame_count: torch.Tensor
    unbatched: bool = False

    estimated = property(lambda self: (self.flags & 1) != 0)
    degenerate = property(lambda self: (self.flags & 2) != 0)


def sample_frame_index(cloud, sample_region):
    """`frame_indices` of the reference (torch_single_view_point_cloud.py:53) per scene, without a sync: cloud (B, 3, N)
    -> (B, N) int32 ascending indices of the points with z > sample_region, then -1, and their number (B,) int64."""
    B, _, N = cloud.shape
    above = cloud[:, 2, :] > sample_region
    count = above.sum(1)
    # a stable sort of "not above" keeps the chosen points in front, each group in ascending index
    order = torch.sort((~above).to(torch.uint8), dim=1, stable=True).indices
    live = torch.arange(N, device=cloud.device).view(1, N) < count.view(B, 1)
    return torch.where(live, order, order.new_full((), -1)).to(torch.int32), count


def estimate_frames(cloud, normals, frame_index=None, frame_count=None, radius=CURVATURE_RADIUS, min_neighbours=5,
                    sample_region=None):
    """The data generator's Darboux frames -- `TorchSingleViewPointCloud._estimate_frame`
    (data_gen/pcd_classes/torch_single_view_point_cloud.py:107-133), which `estimate_frames` (:98-105) loops over the
    sampled points with a kd-tree radius query and an `eigh` each -- for every frame of every scene in one sync-free,
    graph-capturable call -> `DarbouxFrames`, whose `points`, `frames` and `frame_count` are `grade_local_search`'s
    inputs.

    cloud, normals (B, 3, N) fp32, the normals used as given.  One scene may be passed unbatched -- cloud, normals
    (3, N) and frame_index (F,) -- and gets a leading 1: the result is ALWAYS batched (B = 1 then, `unbatched` set,
    as `grade_local_search` does) and frame_count is always (B,).  frame_index (B, F)
    int32 indices into the cloud, a negative one marking a padding row; frame_count (B,) on the device (optional): the
    rows at or past it are padding.  frame_index=None takes the reference's `frame_indices` (:53): the ascending
    indices of the points with z > sample_region (default TABLE_HEIGHT + 0.015 of `LocalSearchConfig`), F = N rows
    padded with -1, and their count.  Per frame: the neighbours with squared distance < radius^2 (the point itself
    included, any number), the covariance of their normals about the projected mean (:122-125), the eigenvector of
    its smallest eigenvalue, columns [-n, -principal, minor] (:126-133).

    Three decisions.  (1) Fewer than min_neighbours neighbours: the identity frame, as the reference leaves it
    (:118-120); `count` tells.  (2) A frame whose eigenvector is parallel to the normal, or whose inputs are not finite
    (NaN in the reference): the zero frame, which `grade_local_search` rejects, and `degenerate`.  (3) The
    eigenvector's sign, which the reference leaves to LAPACK: the largest component of the unnormalised minor axis is
    positive, the lowest index winning a tie.  The other sign turns the frame half a turn about its approach axis,
    which maps the placement at roll theta onto the one at -theta."""
    for name, t in (("cloud", cloud), ("normals", normals)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    if not float(radius) > 0.0:
        raise ValueError("radius must be positive, got %r" % (radius,))
    if int(min_neighbours) < 1:
        raise ValueError("min_neighbours must be at least 1, got %r" % (min_neighbours,))
    if frame_index is not None and (not isinstance(frame_index, torch.Tensor) or frame_index.device.type != "cuda"):
        raise RuntimeError("frame_index must be a CUDA tensor (there is no CPU fallback)")
    unbatched = cloud.dim() == 2
    if unbatched:                       # one scene: (3, N), (3, N), (F,); frame_count stays (1,), as for grade_local_search
        cloud, normals = cloud[None], normals[None]
        frame_index = None if frame_index is None else frame_index[None]
    xyz = _F._f32c(cloud, "cloud")
    nrm = _F._f32c(normals, "normals")
    if xyz.dim() != 3 or xyz.size(1) != 3 or xyz.size(2) < 1:
        raise RuntimeError("cloud must be (B, 3, N)")
    B, _, N = xyz.shape
    if tuple(nrm.shape) != (B, 3, N):
        raise RuntimeError("normals must be (B, 3, N) like cloud")
    dev = xyz.device
    if frame_index is None:
        if frame_count is not None:
            raise RuntimeError("frame_count needs a frame_index")
        if sample_region is None:
            sample_region = LocalSearchConfig().table_height + SAMPLE_REGION_OFFSET
        index, cnt = sample_frame_index(xyz, float(sample_region))
    else:
        if frame_index.dtype != torch.int32:
            raise RuntimeError("frame_index must be int32, got %s" % frame_index.dtype)
        if frame_index.dim() != 2 or frame_index.size(0) != B:
            raise RuntimeError("frame_index must be (B, F)")
        index = frame_index.contiguous()
        cnt = _scene_count(frame_count, B, dev, "frame_count")
    if len({xyz.device, nrm.device, index.device}) != 1:
        raise RuntimeError("cloud, normals and frame_index must live on one device")
    F = index.shape[1]
    frames = torch.empty((B, F, 3, 3), dtype=torch.float32, device=dev)
    points = torch.empty((B, F, 3), dtype=torch.float32, device=dev)
    count = torch.empty((B, F), dtype=torch.int32, device=dev)
    flags = torch.empty((B, F), dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(_cabi.lib().s4g_darboux_frames_workspace_bytes(B, N, F), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_darboux_frames_f32(xyz.data_ptr(), nrm.data_ptr(), index.data_ptr(),
                                                None if cnt is None else cnt.data_ptr(), B, N, F, float(radius),
                                                int(min_neighbours), frames.data_ptr(), points.data_ptr(),
                                                count.data_ptr(), flags.data_ptr(), ws.data_ptr(), nbytes,
                                                _F._stream())
    _cabi.check(rc, "darboux_frames")
    return DarbouxFrames(frames, points, count, flags, index, cnt, unbatched)


def map_cloud_index(valid_index, frame_index):
    """`valid_index` as the reference stores it (:357): the CLOUD index of each valid frame.  valid_index (B, F) frame
    rows padded with -1 (what `grade_local_search` reports), frame_index (B, F) -> (B, F) int32, -1 where padded."""
    live = valid_index >= 0
    got = torch.gather(frame_index, 1, valid_index.clamp(min=0).to(torch.int64))
    return torch.where(live, got, got.new_full((), -1))


NORMAL_MAX_NN = 30                         # data_gen/configs/config.py:31


@dataclass
class MatchedNormals:
    """What `match_normals` returns: device tensors, one column per view point.  `normals` (B, 3, N) fp32, `count`
    (B, N) int32 the number of scene normals averaged (at most max_nn), `flags` (B, N) int32 the kernel's own (bit 0 =
    capped, bit 1 = empty, bit 2 = cancelled, bit 3 = not finite)."""
    normals: torch.Tensor
    count: torch.Tensor
    flags: torch.Tensor
    unbatched: bool = False

    capped = property(lambda self: (self.flags & 1) != 0)
    empty = property(lambda self: (self.flags & 2) != 0)
    cancelled = property(lambda self: (self.flags & 4) != 0)
    nonfinite = property(lambda self: (self.flags & 8) != 0)


def match_normals(cloud, scene_points, scene_normals, camera=None, radius=CURVATURE_RADIUS, max_nn=NORMAL_MAX_NN):
    """The data generator's normal matching -- `TorchSingleViewPointCloud._find_normal`
    (data_gen/pcd_classes/torch_single_view_point_cloud.py:135-150), which loops over the view with one kd-tree
    `search_hybrid_vector_3d(radius, max_nn)` each and then normalises and orients the cloud -- for every view point of
    every scene in one sync-free, graph-capturable call -> `MatchedNormals`, whose `normals` are `estimate_frames`'
    and `label_view`'s input.

    cloud (B, 3, N) fp32 the view; scene_points, scene_normals (B, 3, M) fp32 the dense scene, the normals used as
    given; camera (B, 3) or (3,) (one location for every scene) the camera location `camera_pose[0:3, 3]`, None: no
    orientation.  One view may be passed unbatched -- cloud (3, N), with its scene (3, M) if that is unbatched too --
    and gets a leading 1: the result is ALWAYS batched (`unbatched` set, as `estimate_frames` does).  Per view point:
    the scene points with squared distance < radius^2 (fp32, strict), of them the max_nn smallest by (fp32 squared
    distance, index) -- open3d's hybrid search with the tie order pinned: the lower index wins -- the mean of their
    normals in double, normalised, turned towards the camera, rounded to fp32 once.  No limit on M: the neighbour grid
    is built with the library's radix sort.

    Decisions.  (1) No scene point in the radius: (0, 0, 1), which open3d makes of numpy's NaN mean, then oriented;
    `empty`.  (2) The kept normals cancel to exactly zero: the unit vector towards the camera (zero without a camera);
    `cancelled`.  (3) A view point that is not finite: as (1), not oriented, and `nonfinite`.  (4) A scene point that
    is not finite is never a neighbour.  (5) A kept normal that is not finite: NaN, and `nonfinite`; `estimate_frames`
    then marks the row degenerate."""
    for name, t in (("cloud", cloud), ("scene_points", scene_points), ("scene_normals", scene_normals)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    if not float(radius) > 0.0:
        raise ValueError("radius must be positive, got %r" % (radius,))
    if not 1 <= int(max_nn) <= 64:
        raise ValueError("max_nn must be in [1, 64], got %r" % (max_nn,))
    if camera is not None and (not isinstance(camera, torch.Tensor) or camera.device.type != "cuda"):
        raise RuntimeError("camera must be a CUDA tensor (there is no CPU fallback)")
    unbatched = cloud.dim() == 2
    if unbatched:                       # one view: (3, N); its scene (3, M) gets the leading 1 too, a (1, ...) scene passes
        cloud = cloud[None]
        if scene_points.dim() == 2:
            scene_points, scene_normals = scene_points[None], scene_normals[None]
    xyz = _F._f32c(cloud, "cloud")
    pts = _F._f32c(scene_points, "scene_points")
    nrm = _F._f32c(scene_normals, "scene_normals")
    if xyz.dim() != 3 or xyz.size(1) != 3:
        raise RuntimeError("cloud must be (B, 3, N)")
    B, _, N = xyz.shape
    if pts.dim() != 3 or pts.size(0) != B or pts.size(1) != 3 or pts.size(2) < 1:
        raise RuntimeError("scene_points must be (B, 3, M) with M >= 1")
    M = pts.size(2)
    if tuple(nrm.shape) != (B, 3, M):
        raise RuntimeError("scene_normals must be (B, 3, M) like scene_points")
    cam = None
    if camera is not None:
        cam = _F._f32c(camera, "camera")
        if cam.dim() == 1 and cam.numel() == 3:
            cam = cam.view(1, 3).expand(B, 3)
        if tuple(cam.shape) != (B, 3):
            raise RuntimeError("camera must be (B, 3) or (3,)")
        cam = cam.contiguous()
    if len({xyz.device, pts.device, nrm.device} | ({cam.device} if cam is not None else set())) != 1:
        raise RuntimeError("cloud, scene_points, scene_normals and camera must live on one device")
    dev = xyz.device
    normals = torch.empty((B, 3, N), dtype=torch.float32, device=dev)
    count = torch.empty((B, N), dtype=torch.int32, device=dev)
    flags = torch.empty((B, N), dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(_cabi.lib().s4g_match_normals_workspace_bytes(B, N, M), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_match_normals_f32(xyz.data_ptr(), pts.data_ptr(), nrm.data_ptr(),
                                               None if cam is None else cam.data_ptr(), B, N, M, float(radius),
                                               int(max_nn), normals.data_ptr(), count.data_ptr(), flags.data_ptr(),
                                               ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "match_normals")
    return MatchedNormals(normals, count, flags, unbatched)


NORMAL_RADIUS = 0.01                       # data_gen/configs/config.py: NORMAL_RADIUS


@dataclass
class EstimatedNormals:
    """What `estimate_normals` returns: device tensors, one column per cloud point.  `normals` (B, 3, N) fp32, `count`
    (B, N) int32 the number of kept neighbours (at most max_nn, the point itself among them), `flags` (B, N) int32 the
    kernel's own (bit 0 = capped, bit 1 = few, bit 2 = degenerate, bit 3 = not finite, bit 4 = padding)."""
    normals: torch.Tensor
    count: torch.Tensor
    flags: torch.Tensor
    unbatched: bool = False

    capped = property(lambda self: (self.flags & 1) != 0)
    few = property(lambda self: (self.flags & 2) != 0)
    degenerate = property(lambda self: (self.flags & 4) != 0)
    nonfinite = property(lambda self: (self.flags & 8) != 0)
    padding = property(lambda self: (self.flags & 16) != 0)


def estimate_normals(cloud, camera=None, radius=NORMAL_RADIUS, max_nn=NORMAL_MAX_NN, count=None):
    """The reference's normal estimation -- `PointCloud.estimate_normals` (data_gen/pcd_classes/pointcloud.py:48-60,
    cloud_processor.py:44-52): open3d's `estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))`,
    `normalize_normals` and `orient_normals_towards_camera_location` -- for every point of every cloud in one sync-free,
    graph-capturable call -> `EstimatedNormals`, whose `normals` are the input of `estimate_frames`, `label_view` and
    `label_baseline_view` for a cloud that has none.

    cloud (B, 3, N) fp32; camera (B, 3) or (3,) (one location for every cloud) the camera location, None: no camera;
    count (B,) int32 on the device (optional): the rows of cloud b at or past count[b] (clamped to [0, N]) are padding.
    One cloud may be passed unbatched -- (3, N) -- and gets a leading 1: the result is ALWAYS batched (`unbatched`
    set, as `match_normals` does).  Per point: the live finite points with squared distance < radius^2 (fp32, strict),
    of them the max_nn smallest by (fp32 squared distance, index), the point itself included; their covariance about
    their mean in double; the unit eigenvector of its smallest eigenvalue, turned towards the camera (n . (camera - p)
    >= 0), rounded to fp32 once.  Without a camera, where that product is exactly 0 and where the camera is not finite
    the component of largest magnitude is positive, the lowest axis winning a tie (`estimate_frames`' rule).

    Decisions.  (1) Fewer than 3 kept neighbours: (0, 0, 1), given its sign as above; `few`.  (2) All kept points
    identical, or a solve that gives no direction: the same; `degenerate`.  Collinear neighbours get a unit vector
    perpendicular to their line and no flag.  (3) A point that is not finite: (0, 0, 1) as it stands, count 0,
    `nonfinite`; it is nobody's neighbour and does not slow its cloud down.  (4) More than max_nn points in the radius:
    `capped`.  (5) Padding rows: zero, count 0, `padding`."""
    if not isinstance(cloud, torch.Tensor) or cloud.device.type != "cuda":
        raise RuntimeError("cloud must be a CUDA tensor (there is no CPU fallback)")
    if not float(radius) > 0.0:
        raise ValueError("radius must be positive, got %r" % (radius,))
    if not 1 <= int(max_nn) <= 64:
        raise ValueError("max_nn must be in [1, 64], got %r" % (max_nn,))
    if camera is not None and (not isinstance(camera, torch.Tensor) or camera.device.type != "cuda"):
        raise RuntimeError("camera must be a CUDA tensor (there is no CPU fallback)")
    if count is not None and (not isinstance(count, torch.Tensor) or count.device.type != "cuda"):
        raise RuntimeError("count must be a CUDA tensor (there is no CPU fallback)")
    unbatched = cloud.dim() == 2
    if unbatched:
        cloud = cloud[None]
    xyz = _F._f32c(cloud, "cloud")
    if xyz.dim() != 3 or xyz.size(1) != 3:
        raise RuntimeError("cloud must be (B, 3, N)")
    B, _, N = xyz.shape
    cam = None
    if camera is not None:
        cam = _F._f32c(camera, "camera")
        if cam.dim() == 1 and cam.numel() == 3:
            cam = cam.view(1, 3).expand(B, 3)
        if tuple(cam.shape) != (B, 3):
            raise RuntimeError("camera must be (B, 3) or (3,)")
        cam = cam.contiguous()
    live = None
    if count is not None:
        if count.dtype != torch.int32:
            raise RuntimeError("count must be int32, got %s" % count.dtype)
        if tuple(count.shape) != (B,):
            raise RuntimeError("count must be (B,)")
        live = count.contiguous()
    if len({t.device for t in (xyz, cam, live) if t is not None}) != 1:
        raise RuntimeError("cloud, camera and count must live on one device")
    dev = xyz.device
    normals = torch.empty((B, 3, N), dtype=torch.float32, device=dev)
    cnt = torch.empty((B, N), dtype=torch.int32, device=dev)
    flags = torch.empty((B, N), dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(_cabi.lib().s4g_estimate_normals_workspace_bytes(B, N), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_estimate_normals_f32(xyz.data_ptr(), None if cam is None else cam.data_ptr(),
                                                  None if live is None else live.data_ptr(), B, N, float(radius),
                                                  int(max_nn), normals.data_ptr(), cnt.data_ptr(), flags.data_ptr(),
                                                  ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "estimate_normals")
    return EstimatedNormals(normals, cnt, flags, unbatched)


@dataclass
class ViewLabels:
    """What `label_view` returns: the `LocalSearch` of the view's frames, the `DarbouxFrames` they came from and
    `cloud_index` (B, F): the cloud indices of the valid frames in ascending order, then -1 (`search.count` of them);
    `matched`: the `MatchedNormals` the frames were estimated on, None unless `match_normal` was asked for;
    `estimated`: the `EstimatedNormals` they were estimated on, None unless `estimate_normal` was."""
    search: LocalSearch
    darboux: DarbouxFrames
    cloud_index: torch.Tensor
    matched: MatchedNormals = None
    estimated = None                        # (a plain attribute, set by `label_view`: the constructor's fields stay four)


def label_view(cloud, normals, scene_points, scene_normals, scene_labels, config=None, frame_index=None,
               frame_count=None, radius=CURVATURE_RADIUS, min_neighbours=5, estimate_normal=False, match_normal=False,
               camera=None, max_nn=NORMAL_MAX_NN):
    """`TorchSingleViewPointCloud.run_score(scene, match_normal)` (:182-201): view cloud in, S4G labels out, in one
    sync-free call -- `match_normals` where match_normal is set (:189-190), the sampled indices (:53, z >
    config.table_height + 0.015, unless frame_index is given), `estimate_frames`, then `grade_local_search` on its
    points and frames with its frame count -> `ViewLabels`.  cloud, normals (B, 3, N) are the view; scene_points,
    scene_normals (B, 3, M) and scene_labels (B, M) the dense scene the placements are graded against (the view itself
    in the reference's eval mode).  One unbatched view (3, N) gets a leading 1, with its scene if that is unbatched
    too; the results are always batched.  match_normal=True: `normals` may be None; the view's normals are
    `match_normals(cloud, scene_points, scene_normals, camera, radius, max_nn).normals` (camera (B, 3) or (3,): the
    camera location) and `ViewLabels.matched` holds that result.  estimate_normal=True
    (`TorchSingleViewPointCloud(estimate_normals=True)`, :58-59; exclusive with match_normal): `normals` may be None
    as well; the view's normals are `estimate_normals(cloud, camera, radius, max_nn).normals` and
    `ViewLabels.estimated` holds that result."""
    cfg = config or LocalSearchConfig()
    matched = estimated = None
    if match_normal and estimate_normal:
        raise ValueError("match_normal and estimate_normal exclude each other")
    if estimate_normal:
        estimated = estimate_normals(cloud, camera, radius, max_nn)
        normals = estimated.normals[0] if estimated.unbatched else estimated.normals
    if match_normal:
        matched = match_normals(cloud, scene_points, scene_normals, camera, radius, max_nn)
        normals = matched.normals[0] if isinstance(cloud, torch.Tensor) and cloud.dim() == 2 else matched.normals
    d = estimate_frames(cloud, normals, frame_index, frame_count, radius, min_neighbours,
                        sample_region=cfg.table_height + SAMPLE_REGION_OFFSET)
    if d.unbatched and scene_points.dim() == 2:          # one view against one unbatched scene; a (1, ...) scene passes as is
        scene_points, scene_normals, scene_labels = scene_points[None], scene_normals[None], scene_labels[None]
    s = grade_local_search(d.points, d.frames, scene_points, scene_normals, scene_labels, cfg, d.frame_count)
    out = ViewLabels(s, d, map_cloud_index(s.valid_index, d.frame_index), matched)
    out.estimated = estimated
    return out


CS_MAX_LIST = 4                            # the compiled maximum of each shift list (csrc/contact_search.hip)
FAIL_TABLE, FAIL_FINGER, FAIL_BEHIND, FAIL_LABELS, FAIL_EMPTY, FAIL_NONFINITE = 1, 2, 4, 8, 16, 32


@dataclass
class ContactSearchConfig:
    """The constants of the contact model's label search: the shift lists of
    data_gen/pcd_classes/torch_contact_single_view_point_cloud.py:11-15, the gripper and table constants of
    `LocalSearchConfig` (data_gen/configs/config.py:17,40,50-56,89) and the label of a frame without one
    (`len(NAME_LIST)`, :125)."""
    width_search: tuple = (-0.005, 0.005, 0)
    height_search: tuple = (-0.005, 0.005, 0)
    length_search: tuple = (0,)
    table_height: float = 0.75
    back_collision_margin: float = 0.0
    half_bottom_width: float = 0.057
    bottom_length: float = 0.08
    finger_width: float = 0.023
    half_hand_thickness: float = 0.012
    finger_length: float = 0.09
    table_collision_offset: float = 0.005
    no_label: int = 122

    @property
    def half_bottom_space(self):
        return self.half_bottom_width - self.finger_width

    @property
    def shape(self):
        """(nz, ny, nx): heights, widths and lengths; placement (iz * ny + iy) * nx + ix, the reference's loop order."""
        return len(self.height_search), len(self.width_search), len(self.length_search)

    @property
    def placements(self):
        nz, ny, nx = self.shape
        return nz * ny * nx

    def check(self):
        for name, n in zip(("height_search", "width_search", "length_search"), self.shape):
            if not 1 <= n <= CS_MAX_LIST:
                raise ValueError("%s needs 1..%d entries, got %d" % (name, CS_MAX_LIST, n))

    def tables(self):
        """The bounds the reference compares against, each formed in Python floats and rounded to fp32 ONCE (torch
        compares an fp32 tensor with a Python scalar in fp32) -> dict of fp32 CPU tensors `zlo`, `zhi` (nz), `ylo`,
        `yhi`, `dy` (ny), `xlo`, `xhi` (nx).  The sign of dy in `ylo` / `yhi` (+) and in |y + dy| is the reference's
        (:274-276)."""
        self.check()
        hht, hbs = self.half_hand_thickness, self.half_bottom_space
        f64 = lambda v: torch.tensor(v, dtype=torch.float64).to(torch.float32)      # noqa: E731  (one rounding)
        return {"zlo": f64([-hht + float(d) for d in self.height_search]),
                "zhi": f64([hht + float(d) for d in self.height_search]),
                "ylo": f64([-hbs + float(d) for d in self.width_search]),
                "yhi": f64([hbs + float(d) for d in self.width_search]),
                "dy": f64([float(d) for d in self.width_search]),
                "xlo": f64([-self.bottom_length + float(d) for d in self.length_search]),
                "xhi": f64([self.finger_length + float(d) for d in self.length_search])}


@dataclass
class ContactSearch:
    """What `grade_contact_frames` returns: device tensors, one row per scene frame.  `ints` (B, F, P, 4) = {finger,
    close, behind, multi_label} per placement, `table_i32`, `valid_i32`, `objects_label`, `fail` (B, F) int32 are the
    kernel's own outputs (include/s4g_ops.h has the layout and the bits of `fail`)."""
    ints: torch.Tensor
    table_i32: torch.Tensor
    valid_i32: torch.Tensor
    objects_label: torch.Tensor
    fail: torch.Tensor
    g2l: torch.Tensor
    frame_count: torch.Tensor
    config: ContactSearchConfig
    unbatched: bool = False

    finger = property(lambda self: self.ints[..., 0])
    close = property(lambda self: self.ints[..., 1])
    behind = property(lambda self: self.ints[..., 2])
    multi_label = property(lambda self: self.ints[..., 3] != 0)
    table_collision = property(lambda self: self.table_i32 != 0)
    valid = property(lambda self: self.valid_i32 != 0)


def grade_contact_frames(global_to_local, scene_points, scene_labels, config=None, frame_count=None):
    """The contact model's frame grading -- `TorchPrecomputedSingleViewPointCloud.finger_hand` with
    `_table_collision_check` (data_gen/pcd_classes/torch_contact_single_view_point_cloud.py:236-294), which `run_score`
    (:183-185) loops over every (view point, frame) pair -- for every SCENE frame of every scene in one sync-free,
    graph-capturable call -> `ContactSearch`.  Grading reads `global_to_local` and the scene alone, so a scene frame
    is graded once, whichever view points of whichever views pick it.

    global_to_local (B, F, 4, 4) fp32 rigid transforms (`TorchContactScenePointCloud.global_to_local`); scene_points
    (B, 3, M) fp32; scene_labels (B, M) int32; one unbatched scene gets a leading 1.  frame_count (B,) on the device
    (optional): rows at or past it are not scanned and read invalid.  Per frame P = |height| x |width| x |length|
    placements (9 as shipped), counted in one pass; a frame is valid when the centred gripper box clears the table
    and every placement has no finger point, a close region that is not empty, no close point behind the margin and
    one label.  `objects_label` is the close region's label of the last placement, else `config.no_label`.

    Four decisions.  (1) An empty close region makes the reference raise; here the frame is invalid (`fail` bit 4).
    (2) `local_to_global` is the rigid inverse [R^T | -R^T t] formed in the kernel, not `torch.inverse`;
    global_to_local must be rigid and is not checked.  (3) An entry that is not finite makes the frame invalid (`fail`
    bit 5).  (4) The table verdict covers the centred box only: the reference's nine search matrices alias one
    identity (:18-28)."""
    cfg = config or ContactSearchConfig()
    cfg.check()
    for name, t in (("global_to_local", global_to_local), ("scene_points", scene_points),
                    ("scene_labels", scene_labels)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    unbatched = global_to_local.dim() == 3
    if unbatched:
        global_to_local, scene_points, scene_labels = global_to_local[None], scene_points[None], scene_labels[None]
    xyz, _, lab, B, M, dev = _dense_scene(scene_points, scene_labels, same_device=[("global_to_local", global_to_local)],
                                          size="M", nonempty=True)
    if global_to_local.dtype != torch.float32:
        raise RuntimeError("global_to_local must be float32")
    if global_to_local.dim() != 4 or global_to_local.size(0) != B or tuple(global_to_local.shape[2:]) != (4, 4):
        raise RuntimeError("global_to_local must be (B, F, 4, 4)")
    F = global_to_local.shape[1]
    g2l = global_to_local.contiguous()
    cnt = _scene_count(frame_count, B, dev, "frame_count")
    nz, ny, nx = cfg.shape
    P = cfg.placements
    tb = cfg.tables()
    tables = _small_on_device(torch.cat([tb[k] for k in ("zlo", "zhi", "ylo", "yhi", "dy", "xlo", "xhi")]),
                              torch.float32, dev)
    ints = torch.empty((B, F, P, 4), dtype=torch.int32, device=dev)
    table, valid, label, fail = (torch.empty((B, F), dtype=torch.int32, device=dev) for _ in range(4))
    params = (ctypes.c_float * 10)(cfg.finger_length, cfg.bottom_length, cfg.half_hand_thickness,
                                   cfg.half_bottom_width, cfg.half_bottom_space, cfg.back_collision_margin,
                                   cfg.table_height + cfg.table_collision_offset,
                                   max(abs(float(v)) for v in cfg.length_search),
                                   max(abs(float(v)) for v in cfg.width_search),
                                   max(abs(float(v)) for v in cfg.height_search))
    ws, nbytes = _workspace(_cabi.lib().s4g_contact_search_workspace_bytes(B, M, F, P), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_contact_search_f32(g2l.data_ptr(), xyz.data_ptr(), lab.data_ptr(), B, M, F, nz, ny, nx,
                                                params, int(cfg.no_label), tables.data_ptr(),
                                                None if cnt is None else cnt.data_ptr(), ints.data_ptr(),
                                                table.data_ptr(), valid.data_ptr(), label.data_ptr(), fail.data_ptr(),
                                                ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "contact_search")
    return ContactSearch(ints, table, valid, label, fail, g2l, cnt, cfg, unbatched)


def match_nearest(cloud, scene_points, radius=CURVATURE_RADIUS):
    """The `max_nn = 1` search of `TorchPrecomputedSingleViewPointCloud._find_match` (:142-150) for every view point of
    every scene: cloud (B, 3, N), scene_points (B, 3, M) fp32 -> (B, N) int32, the index of the nearest scene point by
    `match_normals`' rule (fp32 squared distance < radius^2, strict; the lower index wins a tie), -1 where there is
    none or the view point is not finite.  Unbatched inputs get a leading 1."""
    for name, t in (("cloud", cloud), ("scene_points", scene_points)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    if not float(radius) > 0.0:
        raise ValueError("radius must be positive, got %r" % (radius,))
    if cloud.dim() == 2:
        cloud = cloud[None]
        if scene_points.dim() == 2:
            scene_points = scene_points[None]
    xyz = _F._f32c(cloud, "cloud")
    pts = _F._f32c(scene_points, "scene_points")
    if xyz.dim() != 3 or xyz.size(1) != 3:
        raise RuntimeError("cloud must be (B, 3, N)")
    B, _, N = xyz.shape
    if pts.dim() != 3 or pts.size(0) != B or pts.size(1) != 3 or pts.size(2) < 1:
        raise RuntimeError("scene_points must be (B, 3, M) with M >= 1")
    if xyz.device != pts.device:
        raise RuntimeError("cloud and scene_points must live on one device")
    M = pts.size(2)
    nearest = torch.empty((B, N), dtype=torch.int32, device=xyz.device)
    ws, nbytes = _workspace(_cabi.lib().s4g_match_normals_workspace_bytes(B, N, M), xyz.device)
    with torch.cuda.device(xyz.device):
        rc = _cabi.lib().s4g_match_nearest_f32(xyz.data_ptr(), pts.data_ptr(), B, N, M, float(radius),
                                               nearest.data_ptr(), ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "match_nearest")
    return nearest


def frames_by_point(frame_point_index, num_points, frame_count=None):
    """The scene frames of every scene point as a CSR, without a sync: frame_point_index (B, F) int -> (`offsets`
    (B, num_points + 1) int32, `order` (B, F) int32); row i of scene b is order[b, offsets[b, i]:offsets[b, i + 1]],
    the frames whose point is i in ascending frame index -- the order of `np.nonzero(frame_point_index == i)` (:152).
    A stable sort by point; rows at or past frame_count[b] and indices outside [0, num_points) sort behind every point."""
    B, F = frame_point_index.shape
    dev = frame_point_index.device
    key = frame_point_index.to(torch.int64)
    dead = (key < 0) | (key >= num_points)
    if frame_count is not None:
        dead = dead | (torch.arange(F, device=dev).view(1, F) >= frame_count.view(B, 1))
    key = torch.where(dead, key.new_full((), num_points), key)
    skey, order = torch.sort(key, dim=1, stable=True)
    points = torch.arange(num_points + 1, device=dev, dtype=torch.int64).view(1, -1).expand(B, -1).contiguous()
    offsets = torch.searchsorted(skey.contiguous(), points)
    return offsets.to(torch.int32).contiguous(), order.to(torch.int32).contiguous()


@dataclass
class ContactLabels:
    """What `label_contact_view` returns: device tensors, one column per view point.  `nearest` (B, N) int32 the
    matched scene point or -1, `normals` (B, 3, N) fp32, `best_frame` (B, N) int32 the scene frame of a valid point or
    -1, `point_score` (B, N) fp32, `valid_index` (B, N) int32 the valid view points in ascending order then -1,
    `count` (B,) int64; `search`: the `ContactSearch` of the scene frames; `cloud` the noisy view as given."""
    nearest: torch.Tensor
    normals: torch.Tensor
    best_frame: torch.Tensor
    point_score: torch.Tensor
    valid_index: torch.Tensor
    count: torch.Tensor
    search: ContactSearch
    cloud: torch.Tensor
    scene_search_score: torch.Tensor
    scene_antipodal_score: torch.Tensor
    unbatched: bool = False

    valid = property(lambda self: self.best_frame >= 0)

    def _of_best(self, per_frame, fill):
        if per_frame.shape[1] == 0:
            return per_frame.new_full(self.best_frame.shape, fill)
        got = torch.gather(per_frame, 1, self.best_frame.clamp(min=0).to(torch.int64))
        return torch.where(self.best_frame >= 0, got, got.new_full((), fill))

    search_score = property(lambda self: self._of_best(self.scene_search_score, 0.0))
    antipodal_score = property(lambda self: self._of_best(self.scene_antipodal_score, 0.0))
    objects_label = property(lambda self: self._of_best(self.search.objects_label, self.search.config.no_label))

    def frames_of(self, frame=None):
        """`local_to_global` of the scene frames `frame` (B, K) (default: `best_frame`): (B, K, 4, 4) fp32, the rigid
        inverse [R^T | -R^T t] of `global_to_local` (`se3_inverse`; not `torch.inverse`, :120).  Rows whose frame is -1
        are 0."""
        frame = self.best_frame if frame is None else frame
        g2l = self.search.g2l
        B, K = frame.shape
        if g2l.shape[1] == 0:
            return torch.zeros((B, K, 4, 4), dtype=torch.float32, device=g2l.device)
        idx = frame.to(device=g2l.device, dtype=torch.int64)
        g = torch.gather(g2l, 1, idx.clamp(min=0).view(B, K, 1, 1).expand(B, K, 4, 4))
        return torch.where((idx >= 0).view(B, K, 1, 1), se3_inverse(g), torch.zeros((), device=g2l.device))

    def dump(self, b=0):
        """The dictionary of the reference's `dump()` (:217-226) for scene b, in the WORLD frame (the camera transform
        is the caller's, as for `LocalSearch.dump`).  Reads the count on the host."""
        n = int(self.count[b])
        vi = self.valid_index[b, :n].long()
        bf = self.best_frame[b:b + 1, vi]
        return {"search_score": self.search_score[b, vi].cpu().numpy(),
                "antipodal_score": self.antipodal_score[b, vi].cpu().numpy(),
                "valid_frame": self.frames_of(bf)[0].cpu().numpy(),
                "valid_index": vi.cpu().numpy(),
                "point_cloud": self.cloud[b].cpu().numpy(),
                "objects_label": self.objects_label[b, vi].cpu().numpy()}


def label_contact_view(reference_cloud, cloud, scene_points, scene_normals, camera, frame_point_index, search_score,
                       antipodal_score, search=None, global_to_local=None, scene_labels=None, config=None,
                       frame_count=None, radius=CURVATURE_RADIUS):
    """`TorchPrecomputedSingleViewPointCloud.run_score` (data_gen/pcd_classes/torch_contact_single_view_point_cloud.py:
    129-226): view cloud in, contact-model labels out, in one sync-free, graph-capturable call -> `ContactLabels`.

    reference_cloud (B, 3, N) the noise-free view points the match runs on (`reference_cloud[index_in_ref]`); cloud
    (B, 3, N) the noisy view, used for the orientation and returned; scene_points, scene_normals (B, 3, M); camera
    (B, 3) or (3,) the camera location; frame_point_index (B, F) int32 the scene point of each scene frame, in any
    order; search_score, antipodal_score (B, F) fp32 the scene's scores.  search: the `ContactSearch` of the scene's
    frames (`grade_contact_frames`; grade once per scene, select once per view), or None: it is computed from
    global_to_local (B, F, 4, 4), scene_labels (B, M), config and frame_count.  One unbatched view gets a leading 1.

    Per view point: i = the nearest scene point (`match_nearest` on reference_cloud); the normal of i, or (0, 0, 1)
    without one, normalised in double, turned towards the camera seen from the NOISY point, rounded once; the score
    min(log(search) / 6.5, 1) * antipodal of every valid frame of i, folded as the reference folds (:200-206: best
    starts at 0, a frame replaces it unless best > score, so an equal score picks the later frame); valid where the
    best score is positive.  Every frame of a scene point takes part: the reference's ten-frames-per-point buffer is
    not reproduced."""
    for name, t in (("reference_cloud", reference_cloud), ("cloud", cloud), ("scene_points", scene_points),
                    ("scene_normals", scene_normals), ("camera", camera), ("frame_point_index", frame_point_index),
                    ("search_score", search_score), ("antipodal_score", antipodal_score)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    unbatched = cloud.dim() == 2
    if unbatched:
        reference_cloud, cloud = reference_cloud[None], cloud[None]
        if scene_points.dim() == 2:
            scene_points, scene_normals = scene_points[None], scene_normals[None]
            scene_labels = None if scene_labels is None else scene_labels[None]
        if frame_point_index.dim() == 1:
            frame_point_index, search_score, antipodal_score = (frame_point_index[None], search_score[None],
                                                                antipodal_score[None])
            global_to_local = None if global_to_local is None else global_to_local[None]
    ref = _F._f32c(reference_cloud, "reference_cloud")
    xyz = _F._f32c(cloud, "cloud")
    pts = _F._f32c(scene_points, "scene_points")
    nrm = _F._f32c(scene_normals, "scene_normals")
    ss = _F._f32c(search_score, "search_score")
    aps = _F._f32c(antipodal_score, "antipodal_score")
    if xyz.dim() != 3 or xyz.size(1) != 3:
        raise RuntimeError("cloud must be (B, 3, N)")
    B, _, N = xyz.shape
    if tuple(ref.shape) != (B, 3, N):
        raise RuntimeError("reference_cloud must be (B, 3, N) like cloud")
    if pts.dim() != 3 or pts.size(0) != B or pts.size(1) != 3 or pts.size(2) < 1:
        raise RuntimeError("scene_points must be (B, 3, M) with M >= 1")
    M = pts.size(2)
    if tuple(nrm.shape) != (B, 3, M):
        raise RuntimeError("scene_normals must be (B, 3, M) like scene_points")
    if frame_point_index.dtype != torch.int32:
        raise RuntimeError("frame_point_index must be int32, got %s" % frame_point_index.dtype)
    if frame_point_index.dim() != 2 or frame_point_index.size(0) != B:
        raise RuntimeError("frame_point_index must be (B, F)")
    F = frame_point_index.size(1)
    if tuple(ss.shape) != (B, F) or tuple(aps.shape) != (B, F):
        raise RuntimeError("search_score and antipodal_score must be (B, F) like frame_point_index")
    cam = _F._f32c(camera, "camera")
    if cam.dim() == 1 and cam.numel() == 3:
        cam = cam.view(1, 3).expand(B, 3)
    if tuple(cam.shape) != (B, 3):
        raise RuntimeError("camera must be (B, 3) or (3,)")
    cam = cam.contiguous()
    if len({ref.device, xyz.device, pts.device, nrm.device, cam.device, frame_point_index.device, ss.device,
            aps.device}) != 1:
        raise RuntimeError("every input must live on one device")
    dev = xyz.device
    if search is None:
        if global_to_local is None or scene_labels is None:
            raise RuntimeError("without search=, global_to_local and scene_labels are needed to grade the frames")
        search = grade_contact_frames(global_to_local, pts, scene_labels, config, frame_count)
    elif frame_count is None:
        frame_count = search.frame_count
    if tuple(search.valid_i32.shape) != (B, F) or search.valid_i32.device != dev:
        raise RuntimeError("search must hold the (B, F) frames of frame_point_index, on the same device")
    cnt = _scene_count(frame_count, B, dev, "frame_count")
    nearest = match_nearest(ref, pts, radius)
    offsets, order = frames_by_point(frame_point_index, M, cnt)
    normals = torch.empty((B, 3, N), dtype=torch.float32, device=dev)
    best = torch.empty((B, N), dtype=torch.int32, device=dev)
    score = torch.empty((B, N), dtype=torch.float32, device=dev)
    valid_index = torch.empty((B, N), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_contact_select_f32(nearest.data_ptr(), xyz.data_ptr(), nrm.data_ptr(), cam.data_ptr(),
                                                offsets.data_ptr(), order.data_ptr(), search.valid_i32.data_ptr(),
                                                ss.data_ptr(), aps.data_ptr(), B, N, M, F, normals.data_ptr(),
                                                best.data_ptr(), score.data_ptr(), valid_index.data_ptr(),
                                                count.data_ptr(), _F._stream())
    _cabi.check(rc, "contact_select")
    return ContactLabels(nearest, normals, best, score, valid_index, count, search, xyz, ss, aps, unbatched)


CP_MAX_THETA, CP_MAX_SHIFT = 16, 4         # the compiled maxima of csrc/contact_pairs.hip
CP_FAIL_NONFINITE, CP_FAIL_PLANE, CP_FAIL_INDEX = 1, 2, 4
CP_FLAG_PAIRS, CP_FLAG_FRAMES = 1, 2
CP_DEFAULT_PAIRS_PER_POINT = 16            # the default capacities: max_pairs = min(N (N - 1) / 2, 16 N),
CP_DEFAULT_FRAMES_PER_PAIR = 6             # max_frames = min(T, 6) max_pairs (the reference's camera: 6.7 and 3.6)


@dataclass
class ContactPairConfig:
    """The constants of the contact model's per-object data (data_gen/data_generator/
    data_object_contact_point_generator.py:15-18,193,173,209 and data_gen/configs/config.py:38-56): the gripper constants
    of `ContactSearchConfig`, GASKET_RADIUS, COS_THR, THETA_SEARCH in degrees, the shifts of the hand along its
    thickness in the reference's loop order, and the gates."""
    back_collision_margin: float = 0.0
    half_bottom_width: float = 0.057
    bottom_length: float = 0.08
    finger_width: float = 0.023
    half_hand_thickness: float = 0.012
    finger_length: float = 0.09
    gasket_radius: float = 0.012
    cos_threshold: float = 0.95
    theta_search: tuple = tuple(range(0, 360, 30))
    width_shift: tuple = (-0.015, 0.015, 0)
    min_points: float = 50
    back_threshold: float = 0
    finger_threshold: float = 0

    @property
    def half_bottom_space(self):
        return self.half_bottom_width - self.finger_width

    @property
    def max_distance(self):
        return self.half_bottom_space * 2                       # :105, in Python floats

    def check(self):
        if not 1 <= len(self.theta_search) <= CP_MAX_THETA:
            raise ValueError("theta_search needs 1..%d entries, got %d" % (CP_MAX_THETA, len(self.theta_search)))
        if not 1 <= len(self.width_shift) <= CP_MAX_SHIFT:
            raise ValueError("width_shift needs 1..%d entries, got %d" % (CP_MAX_SHIFT, len(self.width_shift)))

    def local_to_local_search(self):
        """`torch.inverse(local_search_to_local)` built as the reference builds it (:29-40): float64 numpy rolls about
        y composed with the move-back of FINGER_LENGTH - GASKET_RADIUS, rounded to fp32, inverted in fp32 on the CPU
        -> (T, 4, 4) fp32 CPU tensor."""
        import numpy as np
        self.check()
        T = len(self.theta_search)
        back = np.eye(4)
        back[0, 3] = -(self.finger_length - self.gasket_radius)
        m = np.tile(np.eye(4), (T, 1, 1))
        for i, th in enumerate(self.theta_search):
            m[i, 0, 0] = np.cos(th / 180 * np.pi)
            m[i, 2, 2] = np.cos(th / 180 * np.pi)
            m[i, 0, 2] = np.sin(th / 180 * np.pi)
            m[i, 2, 0] = -np.sin(th / 180 * np.pi)
        return torch.inverse(torch.tensor(m @ back, dtype=torch.float))

    def tables(self):
        """The device table of `s4g_contact_pair_grade_f32`: rows 0..2 of every roll's matrix, then the lower and the
        upper z bound of every shift, each formed in Python floats and rounded to fp32 once -> (12 T + 2 W,) fp32."""
        hht = self.half_hand_thickness
        z = torch.tensor([-hht + float(d) for d in self.width_shift] + [hht + float(d) for d in self.width_shift],
                         dtype=torch.float64).to(torch.float32)
        return torch.cat([self.local_to_local_search()[:, :3, :].reshape(-1), z])


@dataclass
class ContactPairs:
    """What `contact_pairs` returns: `pairs` (B, max_pairs, 2) int32 in ascending (i, j) then -1, `score` (B, max_pairs)
    fp32, `count` (B,) int64 the exact number of pairs, `flags` (B,) int32 (`CP_FLAG_PAIRS`: the list did not fit)."""
    pairs: torch.Tensor
    score: torch.Tensor
    count: torch.Tensor
    flags: torch.Tensor
    config: ContactPairConfig
    unbatched: bool = False


@dataclass
class ContactPairGrades:
    """What `grade_contact_pairs` returns.  Dense, one row per pair: `counts` (B, P, T, W, 3) int32 = {back, finger,
    close}, `close_plane` (B, P) int32, `score` (B, P, T) fp32, `valid_i32` (B, P, T), `fail` (B, P) int32
    (`CP_FAIL_*`).  The kept frames, `max_frames` rows per object in ascending pair * T + roll: `global_to_local`
    (B, F, 4, 4) fp32, `search_score`, `antipodal_score` (B, F) fp32, `frame_source` (B, F) int32 = pair * T + roll,
    `frame_point_index` (B, F) int32, `frame_count` (B,) int64 the exact number, `flags` (B,) int32
    (`CP_FLAG_FRAMES`: the list did not fit)."""
    counts: torch.Tensor
    close_plane: torch.Tensor
    score: torch.Tensor
    valid_i32: torch.Tensor
    fail: torch.Tensor
    global_to_local: torch.Tensor
    search_score: torch.Tensor
    antipodal_score: torch.Tensor
    frame_source: torch.Tensor
    frame_point_index: torch.Tensor
    frame_count: torch.Tensor
    flags: torch.Tensor
    config: ContactPairConfig
    unbatched: bool = False

    valid = property(lambda self: self.valid_i32 != 0)


def _object_cloud(points, normals, count):
    """points (and normals) (B, 3, N) fp32 on one device, N >= 1; an unbatched cloud gets a leading 1."""
    named = [("points", points)] + ([] if normals is None else [("normals", normals)])
    for name, t in named:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    unbatched = points.dim() == 2
    if unbatched:
        points = points[None]
        normals = None if normals is None else normals[None]
        if isinstance(count, torch.Tensor) and count.dim() == 0:
            count = count[None]
    xyz = _F._f32c(points, "points")
    if xyz.dim() != 3 or xyz.size(1) != 3 or xyz.size(2) < 1:
        raise RuntimeError("points must be (B, 3, N) with N >= 1")
    nrm = None
    if normals is not None:
        nrm = _F._f32c(normals, "normals")
        if tuple(nrm.shape) != tuple(xyz.shape) or nrm.device != xyz.device:
            raise RuntimeError("normals must be (B, 3, N) like points, on the same device")
    cnt = _scene_count(count, xyz.size(0), xyz.device, "count")
    return xyz, nrm, cnt, unbatched


def contact_pairs(points, normals, config=None, count=None, max_pairs=None):
    """`GenerateContactObjectData.cache_contact_pair` (data_object_contact_point_generator.py:103-123) for every object
    of a batch in one sync-free, graph-capturable call -> `ContactPairs`.  points, normals (B, 3, N) fp32, the normals
    of unit length; count (B,) on the device (optional): the points of object b are its first count[b].  The test runs
    in double from the fp32 inputs; the list comes in the order of `np.nonzero(np.triu(...))`.  max_pairs: the rows of
    the padded list (default min(N (N - 1) / 2, 16 N)); `count` stays exact and `flags` says when it did not fit."""
    cfg = config or ContactPairConfig()
    cfg.check()
    xyz, nrm, cnt, unbatched = _object_cloud(points, normals, count)
    B, _, N = xyz.shape
    dev = xyz.device
    if max_pairs is None:
        max_pairs = min(N * (N - 1) // 2, CP_DEFAULT_PAIRS_PER_POINT * N)
    max_pairs = int(max_pairs)
    pairs = torch.empty((B, max_pairs, 2), dtype=torch.int32, device=dev)
    score = torch.empty((B, max_pairs), dtype=torch.float32, device=dev)
    pcount = torch.empty((B,), dtype=torch.int64, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(_cabi.lib().s4g_contact_pairs_workspace_bytes(B, N), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_contact_pairs_f32(xyz.data_ptr(), nrm.data_ptr(), None if cnt is None else cnt.data_ptr(),
                                               B, N, max_pairs, float(cfg.max_distance), float(cfg.cos_threshold),
                                               pairs.data_ptr(), score.data_ptr(), pcount.data_ptr(), flags.data_ptr(),
                                               ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "contact_pairs")
    return ContactPairs(pairs, score, pcount, flags, cfg, unbatched)


def grade_contact_pairs(points, pairs, config=None, count=None, pair_count=None, pair_score=None, max_frames=None):
    """`_estimate_grasp_quality` with `check_collision` and `get_frame_neighbor` (data_object_contact_point_generator.py:
    79-86,125-221) for every pair of every object in one sync-free, graph-capturable call -> `ContactPairGrades`.
    points (B, 3, N) fp32; pairs (B, P, 2) int32 or a `ContactPairs` (its count and score are then the defaults);
    pair_count (B,) on the device (optional): the pairs of object b are its first pair_count[b]; pair_score (B, P) fp32
    (optional) becomes `antipodal_score`.  max_frames: the rows of the frame list (default min(T, 6) P).

    Four decisions.  (1) The frame of a pair is formed in double and its rigid inverse analytically, not by
    `torch.inverse` in fp32.  (2) A pair whose frame is not finite gets no frame and `CP_FAIL_NONFINITE`; the reference
    would propagate NaN.  (3) `antipodal_score` is fp32; the reference keeps float64.  (4) Thresholds and search lists
    are configuration, at most 16 rolls and 4 shifts."""
    cfg = config or (pairs.config if isinstance(pairs, ContactPairs) else ContactPairConfig())
    cfg.check()
    if isinstance(pairs, ContactPairs):
        pair_count = pairs.count if pair_count is None else pair_count
        pair_score = pairs.score if pair_score is None else pair_score
        pairs = pairs.pairs
    xyz, _, cnt, unbatched = _object_cloud(points, None, count)
    B, _, N = xyz.shape
    dev = xyz.device
    if not isinstance(pairs, torch.Tensor) or pairs.device != dev or pairs.dtype != torch.int32:
        raise RuntimeError("pairs must be an int32 tensor on the device of points")
    if pairs.dim() == 2:
        pairs = pairs[None]
        pair_score = pair_score[None] if pair_score is not None and pair_score.dim() == 1 else pair_score
    if pairs.dim() != 3 or pairs.size(0) != B or pairs.size(2) != 2:
        raise RuntimeError("pairs must be (B, P, 2)")
    pairs = pairs.contiguous()
    P = pairs.size(1)
    if pair_score is not None:
        pair_score = _F._f32c(pair_score, "pair_score")
        if tuple(pair_score.shape) != (B, P) or pair_score.device != dev:
            raise RuntimeError("pair_score must be (B, P) on the device of points")
    pcnt = _scene_count(pair_count, B, dev, "pair_count")
    T, W = len(cfg.theta_search), len(cfg.width_shift)
    if max_frames is None:
        max_frames = min(T, CP_DEFAULT_FRAMES_PER_PAIR) * P
    F = int(max_frames)
    tables = _small_on_device(cfg.tables(), torch.float32, dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)            # noqa: E731
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
    out = ContactPairGrades(i32(B, P, T, W, 3), i32(B, P), f32(B, P, T), i32(B, P, T), i32(B, P), f32(B, F, 4, 4),
                            f32(B, F), f32(B, F), i32(B, F), i32(B, F),
                            torch.empty((B,), dtype=torch.int64, device=dev), i32(B), cfg, unbatched)
    once = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32))    # noqa: E731  (one rounding)
    params = (ctypes.c_float * 5)(once(cfg.half_bottom_width), once(cfg.half_bottom_space),
                                  once(cfg.back_collision_margin), once(cfg.bottom_length), once(cfg.finger_length))
    gates = (ctypes.c_double * 3)(float(cfg.min_points), float(cfg.back_threshold), float(cfg.finger_threshold))
    ws, nbytes = _workspace(_cabi.lib().s4g_contact_pair_grade_workspace_bytes(B, N, P, T, W), dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()             # noqa: E731
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_contact_pair_grade_f32(
            xyz.data_ptr(), ptr(cnt), ptr(pairs), ptr(pair_score), ptr(pcnt), B, N, P, T, W, params, gates,
            tables.data_ptr(), F, ptr(out.counts), ptr(out.close_plane), ptr(out.score), ptr(out.valid_i32),
            ptr(out.fail), ptr(out.global_to_local), ptr(out.search_score), ptr(out.antipodal_score),
            ptr(out.frame_source), ptr(out.frame_point_index), out.frame_count.data_ptr(), out.flags.data_ptr(),
            ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "contact_pair_grade")
    return out


@dataclass
class ObjectContactFrames:
    """What `label_contact_object` returns: the kept frames of every object -- `global_to_local` (B, F, 4, 4),
    `search_score`, `antipodal_score` (B, F) fp32, `frame_point_index` (B, F) int32, `frame_count` (B,) int64 -- with
    the `pairs` (`ContactPairs`) and `grades` (`ContactPairGrades`) behind them, `flags` (B,) int32 the union of
    theirs, and the cloud as given."""
    global_to_local: torch.Tensor
    search_score: torch.Tensor
    antipodal_score: torch.Tensor
    frame_point_index: torch.Tensor
    frame_count: torch.Tensor
    flags: torch.Tensor
    pairs: ContactPairs
    grades: ContactPairGrades
    points: torch.Tensor
    normals: torch.Tensor
    count: torch.Tensor
    unbatched: bool = False

    def dump(self, b=0):
        """The dictionary the reference pickles per object (:65-74) for object b, as numpy.  Reads the counts on the
        host."""
        n = self.points.shape[2] if self.count is None else int(self.count[b])
        f = min(int(self.frame_count[b]), self.global_to_local.shape[1])
        return {"cloud": self.points[b, :, :n].t().cpu().numpy(),
                "normal": self.normals[b, :, :n].t().cpu().numpy(),
                "global_to_local": self.global_to_local[b, :f].cpu().numpy(),
                "search_score": self.search_score[b, :f].cpu().numpy(),
                "antipodal_score": self.antipodal_score[b, :f].cpu().numpy(),
                "frame_point_index": self.frame_point_index[b, :f].cpu().numpy()}


def label_contact_object(points, normals, config=None, count=None, max_pairs=None, max_frames=None):
    """`GenerateContactObjectData.run_loop` from the sampled cloud on (data_object_contact_point_generator.py:65-74):
    object cloud in, the contact model's per-object frames out, in one sync-free, graph-capturable call on the
    library's stream -> `ObjectContactFrames`.  `contact_pairs` then `grade_contact_pairs`; see both for the
    arguments, the capacities and the four decisions."""
    cfg = config or ContactPairConfig()
    prs = contact_pairs(points, normals, cfg, count, max_pairs)
    xyz, nrm, cnt, unbatched = _object_cloud(points, normals, count)
    g = grade_contact_pairs(xyz, prs, cfg, cnt, max_frames=max_frames)
    return ObjectContactFrames(g.global_to_local, g.search_score, g.antipodal_score, g.frame_point_index,
                               g.frame_count, prs.flags | g.flags, prs, g, xyz, nrm, cnt, unbatched)


def quaternion_matrix(q):
    """A (w, x, y, z) quaternion -> the 3 x 3 rotation, as `transforms3d.quaternions.quat2mat` forms it (float64; a
    quaternion shorter than the float epsilon gives the identity)."""
    w, x, y, z = (float(v) for v in q)
    nq = w * w + x * x + y * y + z * z
    if nq < 2.220446049250313e-16:
        return torch.eye(3, dtype=torch.float64)
    s = 2.0 / nq
    X, Y, Z = x * s, y * s, z * s
    wX, wY, wZ, xX, xY, xZ, yY, yZ, zZ = w * X, w * Y, w * Z, x * X, x * Y, x * Z, y * Y, y * Z, z * Z
    return torch.tensor([[1.0 - (yY + zZ), xY - wZ, xZ + wY],
                         [xY + wZ, 1.0 - (xX + zZ), yZ - wX],
                         [xZ - wY, yZ + wX, 1.0 - (xX + yY)]], dtype=torch.float64)


def pose_matrix(pose):
    """A pose as the scene generator keeps it -- (x, y, z, qw, qx, qy, qz) -> 4 x 4 float64 (:58-62)."""
    t = torch.as_tensor(pose, dtype=torch.float64)
    if tuple(t.shape) != (7,):
        raise ValueError("a pose is (x, y, z, qw, qx, qy, qz)")
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = quaternion_matrix(t[3:].tolist())
    m[:3, 3] = t[:3].cpu()
    return m


@dataclass
class ContactScene:
    """What `compose_contact_scene` returns, one scene: `points`, `normals` (3, M) fp32, `labels` (M,) int32,
    `global_to_local` (F, 4, 4) fp32, `search_score`, `antipodal_score` (F,) fp32, `frame_point_index` (F,) int32 into
    the scene's points."""
    points: torch.Tensor
    normals: torch.Tensor
    labels: torch.Tensor
    global_to_local: torch.Tensor
    search_score: torch.Tensor
    antipodal_score: torch.Tensor
    frame_point_index: torch.Tensor


def compose_contact_scene(objects, poses, labels=None):
    """`GenerateContactScene.generate_single_scene` (data_gen/data_generator/data_contact_scene_generator.py:57-100) in
    torch on the device: objects, a list of (`ObjectContactFrames`, b) or of unbatched `ObjectContactFrames`; poses,
    one (x, y, z, qw, qx, qy, qz) each; labels, one int each (default 0, 1, ...).  Points and normals
    are moved by the pose, global_to_local becomes global_to_local @ inverse(pose), frame_point_index is offset by the
    running point count, everything is concatenated -> `ContactScene`, which goes straight into
    `grade_contact_frames` / `label_contact_view`.  Reads every object's counts on the host."""
    if len(objects) != len(poses) or not objects:
        raise ValueError("one pose per object, at least one object")
    parts = {k: [] for k in ("points", "normals", "labels", "g2l", "search", "antipodal", "index")}
    offset = 0
    for k, (obj, pose) in enumerate(zip(objects, poses)):
        obj, b = obj if isinstance(obj, tuple) else (obj, 0)
        dev = obj.points.device
        n = obj.points.shape[2] if obj.count is None else int(obj.count[b])
        f = min(int(obj.frame_count[b]), obj.global_to_local.shape[1])
        m = pose_matrix(pose)
        m32 = m.to(torch.float32).to(dev)
        inv32 = torch.linalg.inv(m).to(torch.float32).to(dev)
        parts["points"].append(m32[:3, :3] @ obj.points[b, :, :n] + m32[:3, 3:])
        parts["normals"].append(m32[:3, :3] @ obj.normals[b, :, :n])
        parts["labels"].append(torch.full((n,), k if labels is None else int(labels[k]), dtype=torch.int32, device=dev))
        parts["g2l"].append(obj.global_to_local[b, :f] @ inv32)
        parts["search"].append(obj.search_score[b, :f])
        parts["antipodal"].append(obj.antipodal_score[b, :f])
        parts["index"].append(obj.frame_point_index[b, :f] + offset)
        offset += n
    return ContactScene(torch.cat(parts["points"], 1).contiguous(), torch.cat(parts["normals"], 1).contiguous(),
                        torch.cat(parts["labels"]), torch.cat(parts["g2l"]).contiguous(), torch.cat(parts["search"]),
                        torch.cat(parts["antipodal"]), torch.cat(parts["index"]).to(torch.int32))


DO_MAX_DEPTHS, DO_MAX_ANGLES, DO_MAX_SHIFTS = 8, 16, 4     # the compiled maxima of csrc/darboux_object.hip
DO_MAX_POINTS = 65536                      # the frame kernel's cell grid (csrc/grid.h: GR_MAX_POINTS)
DO_FLAG_ESTIMATED, DO_FLAG_DEGENERATE, DO_FLAG_FEW = 1, 2, 4


@dataclass
class DarbouxObjectConfig:
    """The constants of the curvature model's per-object data (data_gen/data_generator/data_object_darboux_generator.py
    and data_gen/configs/config.py:23-56): those of `LocalSearchConfig` that `finger_hand_view` reads, the shifts of the
    hand along its thickness in the reference's loop order (:181), CURVATURE_RADIUS and the neighbour floor (:72,75)."""
    num_points_threshold: float = 8
    length_search: tuple = (-0.08, -0.06, -0.04, -0.02)
    theta_search_deg: tuple = tuple(range(-90, 90, 15))
    shift_search: tuple = (-0.02, 0.02, 0)
    back_collision_threshold: float = 0 * math.sqrt(8)
    back_collision_margin: float = 0.0
    finger_collision_threshold: float = 0
    close_region_min_points: float = 10
    neighbor_depth: float = 0.005
    half_bottom_width: float = 0.057
    bottom_length: float = 0.08
    finger_width: float = 0.023
    half_hand_thickness: float = 0.012
    finger_length: float = 0.09
    radius: float = CURVATURE_RADIUS
    min_neighbours: int = 5

    @property
    def half_bottom_space(self):
        return self.half_bottom_width - self.finger_width

    @property
    def shape(self):
        """(L, T, S): depths, rolls per depth, shifts."""
        return len(self.length_search), len(self.theta_search_deg), len(self.shift_search)

    def check(self):
        L, T, S = self.shape
        if not (1 <= L <= DO_MAX_DEPTHS and 1 <= T <= DO_MAX_ANGLES and 1 <= S <= DO_MAX_SHIFTS):
            raise ValueError("need 1..%d depths, 1..%d angles and 1..%d shifts, got %d, %d and %d"
                             % (DO_MAX_DEPTHS, DO_MAX_ANGLES, DO_MAX_SHIFTS, L, T, S))
        if not float(self.radius) > 0.0:
            raise ValueError("radius must be positive, got %r" % (self.radius,))
        if int(self.min_neighbours) < 1:
            raise ValueError("min_neighbours must be at least 1, got %r" % (self.min_neighbours,))

    def tables(self):
        """`LocalSearchConfig.tables` for the depths and rolls, plus the z window of every shift: `zlo`, `zhi` (S) =
        -HALF_HAND_THICKNESS + dz, HALF_HAND_THICKNESS + dz in Python floats, rounded to fp32 once (:183-184)."""
        self.check()
        tb = LocalSearchConfig(length_search=tuple(self.length_search), theta_search_deg=tuple(self.theta_search_deg),
                               bottom_length=self.bottom_length, finger_length=self.finger_length).tables()
        hht = self.half_hand_thickness
        tb["zlo"] = torch.tensor([-hht + float(d) for d in self.shift_search], dtype=torch.float64).to(torch.float32)
        tb["zhi"] = torch.tensor([hht + float(d) for d in self.shift_search], dtype=torch.float64).to(torch.float32)
        return tb


@dataclass
class ObjectFrames:
    """What `estimate_object_frames` returns, one row per point: `frames`, `inv_frames` (B, N, 3, 3) fp32 with the axes
    as columns, `neighbours` (B, N) int32, `flags` (B, N) int32 (`DO_FLAG_*`)."""
    frames: torch.Tensor
    inv_frames: torch.Tensor
    neighbours: torch.Tensor
    flags: torch.Tensor
    unbatched: bool = False

    estimated = property(lambda self: (self.flags & DO_FLAG_ESTIMATED) != 0)
    degenerate = property(lambda self: (self.flags & DO_FLAG_DEGENERATE) != 0)


@dataclass
class ObjectGrades:
    """What `grade_object_frames` returns, direction 0 = `frames`, 1 = `inv_frames`: `search_score` int32 and
    `antipodal_score` fp32 (B, F, 2, L, T), `counts` (B, F, 2, L, T, S, 3) int32 = {back, finger, close}, `slab_count`
    (B, F, 2, L) int32, `fail_i32` (B, F, 2)."""
    search_score: torch.Tensor
    antipodal_score: torch.Tensor
    counts: torch.Tensor
    slab_count: torch.Tensor
    fail_i32: torch.Tensor
    config: DarbouxObjectConfig
    unbatched: bool = False

    fail = property(lambda self: self.fail_i32 != 0)


def estimate_object_frames(points, normals, count=None, config=None):
    """`GenerateDarbouxObjectData._estimate_frame` (data_gen/data_generator/data_object_darboux_generator.py:62-92),
    which loops over the points with a kd-tree radius query and an `eigh` each, for every point of every object in one
    sync-free, graph-capturable call -> `ObjectFrames`.  points, normals (B, 3, N) fp32, N <= 65 536; an unbatched
    cloud gets a leading 1; count (B,) on the device (optional): the points of object b are its first count[b], the
    other rows read zero frames.  Neighbours: squared distance < radius^2 in fp32, the point itself included.

    Decision 3 of the per-object stage: `M = np.eye(3) - normal.T @ normal` (:80) has a 1-D `normal`, so it is the
    identity with the SCALAR n.n taken off every entry, not the projector of the view class; it is reproduced as
    written, with n the normalised mean of the neighbours' normals and everything up to the covariance in double (the
    reference's shipped object data was made this way).  frame = [-n, -principal, minor], inv_frame = [n, principal,
    minor].  Below `min_neighbours` both are ZERO (:75-78), not the identity the view class leaves.  The eigenvector's
    sign follows `estimate_frames`; a degenerate or non-finite row gives zero frames and `DO_FLAG_DEGENERATE`."""
    cfg = config or DarbouxObjectConfig()
    cfg.check()
    xyz, nrm, cnt, unbatched = _object_cloud(points, normals, count)
    B, _, N = xyz.shape
    if N > DO_MAX_POINTS:
        raise ValueError("an object cloud holds at most %d points, got %d" % (DO_MAX_POINTS, N))
    dev = xyz.device
    if cnt is not None:
        # the columns past count are binned with the points (never read as neighbours): fold them onto the object's
        # own points, so that they are finite and spread over its cells
        col = torch.arange(N, device=dev).view(1, N)
        src = torch.where(col < cnt.view(B, 1), col, col % cnt.clamp(min=1).view(B, 1))
        xyz = torch.gather(xyz, 2, src.view(B, 1, N).expand(B, 3, N)).contiguous()
    out = ObjectFrames(torch.empty((B, N, 3, 3), dtype=torch.float32, device=dev),
                       torch.empty((B, N, 3, 3), dtype=torch.float32, device=dev),
                       torch.empty((B, N), dtype=torch.int32, device=dev),
                       torch.empty((B, N), dtype=torch.int32, device=dev), unbatched)
    ws, nbytes = _workspace(_cabi.lib().s4g_darboux_object_frames_workspace_bytes(B, N), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_darboux_object_frames_f32(
            xyz.data_ptr(), nrm.data_ptr(), None if cnt is None else cnt.data_ptr(), B, N, float(cfg.radius),
            int(cfg.min_neighbours), out.frames.data_ptr(), out.inv_frames.data_ptr(), out.neighbours.data_ptr(),
            out.flags.data_ptr(), ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "darboux_object_frames")
    return out


def _object_grade_args(cfg):
    """(params9 as a ctypes array, the table tensor on the CPU) of `s4g_darboux_object_grade_f32`."""
    tb = cfg.tables()
    zmax = cfg.half_hand_thickness + max(abs(float(d)) for d in cfg.shift_search)
    params = (ctypes.c_float * 9)(cfg.half_bottom_width, cfg.half_bottom_space, cfg.back_collision_margin,
                                  cfg.back_collision_threshold, cfg.finger_collision_threshold,
                                  cfg.close_region_min_points, cfg.neighbor_depth, cfg.num_points_threshold, zmax)
    return params, torch.cat([tb["depth"], tb["lo"], tb["hi"], tb["cos"], tb["sin"], tb["zlo"], tb["zhi"]])


def grade_object_frames(points, normals, frames, inv_frames, config=None, count=None, frame_index=None):
    """`GenerateDarbouxObjectData._estimate_grasp_quality` with `finger_hand_view` and `_antipodal_score`
    (data_object_darboux_generator.py:94-247): every frame and its opposite frame against the object's own cloud, L
    depths x T rolls x S shifts each, for every frame of every object in one sync-free, graph-capturable call ->
    `ObjectGrades`.  points, normals (B, 3, N) fp32; frames, inv_frames (B, F, 3, 3) fp32 with the axes as columns;
    frame_index (B, F) int32 on the device (optional): the point each frame sits at (default: F = N, frame f at point
    f; an index outside the object fails the row); count (B,) as for `estimate_object_frames`.

    Decisions (INTEGRATION.md has all five).  (1) The accumulator pairs of :179-180 -- `a, b = torch.zeros(1, ...)`,
    which raises as written -- are two fp32 scalars that start at 0.  (2) A zero (mean |entry| < 1e-6) or non-finite
    frame gets zero scores and `fail`; the reference raises on the early return of :137.  (4) Global -> local is
    [R^T | -R^T p], not `torch.inverse` in fp32.  (5) Everything else as written, in the reference's order: no table
    gate and no label gate; a depth whose slab holds fewer than NUM_POINTS_THRESHOLD points leaves its placements 0;
    shifts in the order given with the window (-HHT + dz, HHT + dz); per shift the gates back > threshold, finger >
    threshold, close < CLOSE_REGION_MIN_POINTS; `close_region_point_num` is overwritten by every shift that passes the
    two collision gates and `single_antipodal` by every shift that passes all three, and the results are
    min(temp_search, close_region_point_num) and min(temp_antipodal, single_antipodal): the last-shift quirk that
    `grade_contact_pairs` carries for its own class; `temp += n / 3` in fp32 in shift order; `search_score` is int32 by
    truncation; a close region whose points share one y gives a NaN antipodal score that propagates."""
    cfg = config or DarbouxObjectConfig()
    cfg.check()
    xyz, nrm, cnt, unbatched = _object_cloud(points, normals, count)
    B, _, N = xyz.shape
    dev = xyz.device
    for name, t in (("frames", frames), ("inv_frames", inv_frames)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    if frames.dim() == 3:
        frames, inv_frames = frames[None], inv_frames[None]
        frame_index = frame_index[None] if frame_index is not None and frame_index.dim() == 1 else frame_index
    frm, inv = _F._f32c(frames, "frames"), _F._f32c(inv_frames, "inv_frames")
    if frm.dim() != 4 or frm.size(0) != B or tuple(frm.shape[2:]) != (3, 3) or frm.device != dev:
        raise RuntimeError("frames must be (B, F, 3, 3) on the device of points")
    if tuple(inv.shape) != tuple(frm.shape) or inv.device != dev:
        raise RuntimeError("inv_frames must be (B, F, 3, 3) like frames")
    F = frm.size(1)
    if frame_index is None:
        if F != N:
            raise RuntimeError("without a frame_index there is one frame per point: frames must be (B, N, 3, 3)")
    else:
        if not isinstance(frame_index, torch.Tensor) or frame_index.device != dev or frame_index.dtype != torch.int32:
            raise RuntimeError("frame_index must be an int32 tensor on the device of points")
        if tuple(frame_index.shape) != (B, F):
            raise RuntimeError("frame_index must be (B, F)")
        frame_index = frame_index.contiguous()
    L, T, S = cfg.shape
    params, table = _object_grade_args(cfg)
    tables = _small_on_device(table, torch.float32, dev)
    out = ObjectGrades(torch.empty((B, F, 2, L, T), dtype=torch.int32, device=dev),
                       torch.empty((B, F, 2, L, T), dtype=torch.float32, device=dev),
                       torch.empty((B, F, 2, L, T, S, 3), dtype=torch.int32, device=dev),
                       torch.empty((B, F, 2, L), dtype=torch.int32, device=dev),
                       torch.empty((B, F, 2), dtype=torch.int32, device=dev), cfg, unbatched)
    ws, nbytes = _workspace(_cabi.lib().s4g_darboux_object_grade_workspace_bytes(B, N, F, L, T, S), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_darboux_object_grade_f32(
            xyz.data_ptr(), nrm.data_ptr(), None if cnt is None else cnt.data_ptr(), frm.data_ptr(), inv.data_ptr(),
            None if frame_index is None else frame_index.data_ptr(), B, N, F, L, T, S, params, tables.data_ptr(),
            out.search_score.data_ptr(), out.antipodal_score.data_ptr(), out.counts.data_ptr(),
            out.slab_count.data_ptr(), out.fail_i32.data_ptr(), ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "darboux_object_grade")
    return out


@dataclass
class ObjectDarbouxData:
    """What `label_darboux_object` returns: the cloud as given (`points`, `normals` (B, 3, N), `count` (B,) or None),
    its `frames` (`ObjectFrames`) and their `grades` (`ObjectGrades`)."""
    points: torch.Tensor
    normals: torch.Tensor
    count: torch.Tensor
    frames: ObjectFrames
    grades: ObjectGrades
    unbatched: bool = False

    def dump(self, b=0):
        """The dictionary the reference pickles per object (:50-57, :125-128) for object b, as numpy.  Reads the count
        on the host."""
        n = self.points.shape[2] if self.count is None else int(self.count[b])
        g = self.grades
        return {"cloud": self.points[b, :, :n].t().cpu().numpy(),
                "normal": self.normals[b, :, :n].t().cpu().numpy(),
                "frame": self.frames.frames[b, :n].cpu().numpy(),
                "inv_frame": self.frames.inv_frames[b, :n].cpu().numpy(),
                "search_score": g.search_score[b, :n, 0].cpu().numpy(),
                "inv_search_score": g.search_score[b, :n, 1].cpu().numpy(),
                "antipodal_score": g.antipodal_score[b, :n, 0].cpu().numpy(),
                "inv_antipodal_score": g.antipodal_score[b, :n, 1].cpu().numpy()}


def label_darboux_object(points, normals, config=None, count=None):
    """`GenerateDarbouxObjectData.run_loop` from the sampled cloud on (data_object_darboux_generator.py:52-57): object
    cloud in, every point's Darboux frame, its opposite frame and the grasp scores of both out, in one sync-free,
    graph-capturable call on the library's stream -> `ObjectDarbouxData`.  `estimate_object_frames` then
    `grade_object_frames`; see both for the arguments and the decisions."""
    cfg = config or DarbouxObjectConfig()
    xyz, nrm, cnt, unbatched = _object_cloud(points, normals, count)
    fr = estimate_object_frames(xyz, nrm, cnt, cfg)
    g = grade_object_frames(xyz, nrm, fr.frames, fr.inv_frames, cfg, cnt)
    fr.unbatched = g.unbatched = unbatched
    return ObjectDarbouxData(xyz, nrm, cnt, fr, g, unbatched)


@dataclass
class DarbouxScene:
    """What `compose_darboux_scene` returns, one scene of M points: `points`, `normals` (3, M) fp32, `labels` (M,)
    int32, `frames`, `inv_frames` (M, 3, 3) fp32, `search_score`, `inv_search_score` (M, L, T) int32,
    `antipodal_score`, `inv_antipodal_score` (M, L, T) fp32."""
    points: torch.Tensor
    normals: torch.Tensor
    labels: torch.Tensor
    frames: torch.Tensor
    inv_frames: torch.Tensor
    search_score: torch.Tensor
    inv_search_score: torch.Tensor
    antipodal_score: torch.Tensor
    inv_antipodal_score: torch.Tensor

    def dump(self):
        """The dictionary the reference pickles per scene (data_scene_generator.py:105-107), as numpy, without `color`."""
        return {"cloud": self.points.t().cpu().numpy(), "frame": self.frames.cpu().numpy(),
                "label": self.labels.cpu().numpy(), "normal": self.normals.t().cpu().numpy(),
                "inv_frame": self.inv_frames.cpu().numpy(), "search_score": self.search_score.cpu().numpy(),
                "antipodal_score": self.antipodal_score.cpu().numpy(),
                "inv_search_score": self.inv_search_score.cpu().numpy(),
                "inv_antipodal_score": self.inv_antipodal_score.cpu().numpy()}


def compose_darboux_scene(objects, poses, labels=None):
    """`GenerateDarbouxScene.generate_single_scene` (data_gen/data_generator/data_scene_generator.py:59-107) in torch
    on the device: objects, a list of (`ObjectDarbouxData`, b) or of `ObjectDarbouxData` (object 0); poses, one
    (x, y, z, qw, qx, qy, qz) each; labels, one int each (default 0, 1, ...).  Points are moved by the pose, normals and
    both frame sets by its rotation (in fp32; the reference keeps float64), the four score arrays and the labels are
    concatenated -> `DarbouxScene`.  Reads every object's count on the host."""
    if len(objects) != len(poses) or not objects:
        raise ValueError("one pose per object, at least one object")
    keys = ("points", "normals", "labels", "frames", "inv_frames", "search", "inv_search", "antipodal", "inv_antipodal")
    parts = {k: [] for k in keys}
    for k, (obj, pose) in enumerate(zip(objects, poses)):
        obj, b = obj if isinstance(obj, tuple) else (obj, 0)
        dev = obj.points.device
        n = obj.points.shape[2] if obj.count is None else int(obj.count[b])
        m32 = pose_matrix(pose).to(torch.float32).to(dev)
        rot = m32[:3, :3]
        parts["points"].append(rot @ obj.points[b, :, :n] + m32[:3, 3:])
        parts["normals"].append(rot @ obj.normals[b, :, :n])
        parts["labels"].append(torch.full((n,), k if labels is None else int(labels[k]), dtype=torch.int32, device=dev))
        parts["frames"].append(torch.matmul(rot, obj.frames.frames[b, :n]))
        parts["inv_frames"].append(torch.matmul(rot, obj.frames.inv_frames[b, :n]))
        parts["search"].append(obj.grades.search_score[b, :n, 0])
        parts["inv_search"].append(obj.grades.search_score[b, :n, 1])
        parts["antipodal"].append(obj.grades.antipodal_score[b, :n, 0])
        parts["inv_antipodal"].append(obj.grades.antipodal_score[b, :n, 1])
    return DarbouxScene(torch.cat(parts["points"], 1).contiguous(), torch.cat(parts["normals"], 1).contiguous(),
                        torch.cat(parts["labels"]), torch.cat(parts["frames"]).contiguous(),
                        torch.cat(parts["inv_frames"]).contiguous(), torch.cat(parts["search"]).contiguous(),
                        torch.cat(parts["inv_search"]).contiguous(), torch.cat(parts["antipodal"]).contiguous(),
                        torch.cat(parts["inv_antipodal"]).contiguous())


_SCENE_FIELDS = ("points", "normals", "labels", "frames", "inv_frames", "search_score", "inv_search_score",
                 "antipodal_score", "inv_antipodal_score")


@dataclass
class PrecomputedViewConfig:
    """The constants of the fast pipeline's view stage (torch_precomputed_single_view_point_cloud.py): the thresholds
    of `magic_formula` (:181-182), the validity line of `finger_hand` (:384-385), SAMPLE_REGION (None: table_height +
    SAMPLE_REGION_OFFSET of `search`) and the local search's own constants.  search_threshold=None switches that
    threshold off (the mask is the antipodal threshold alone, as `TorchPrecomputedBaselinePointCloud.magic_formula` has
    it): -inf goes to the kernel, and an int32 score > -inf is true in double."""
    search_threshold: float = 50
    antipodal_threshold: float = 0.3
    valid_search_min: float = 1
    valid_antipodal_min: float = 0.1
    sample_region: float = None
    search: LocalSearchConfig = None

    def __post_init__(self):
        if self.search is None:
            self.search = LocalSearchConfig()

    @property
    def region(self):
        return self.search.table_height + SAMPLE_REGION_OFFSET if self.sample_region is None else self.sample_region


@dataclass
class PrecomputedMatch:
    """What `match_scene_frames` returns: device tensors, one row per view point.  `nearest` (B, N) int32 the matched
    scene point or -1, `normals` (B, 3, N) fp32, `flipped` (B, N) bool, `frames` (B, N, 3, 3) fp32, `pre_search`
    (B, N, L, T) int32, `pre_antipodal` (B, N, L, T) fp32, `mask` (B, N, L, T) bool (`all_frame_bool`), `candidate`
    (B, N) bool, `frame_index` (B, N) int32 the candidates in ascending order then -1, `frame_count` (B,) int64;
    `cloud` the noisy view as given."""
    nearest: torch.Tensor
    normals: torch.Tensor
    flipped_i32: torch.Tensor
    frames: torch.Tensor
    pre_search: torch.Tensor
    pre_antipodal: torch.Tensor
    mask: torch.Tensor
    candidate_i32: torch.Tensor
    frame_index: torch.Tensor
    frame_count: torch.Tensor
    cloud: torch.Tensor
    config: PrecomputedViewConfig
    unbatched: bool = False

    flipped = property(lambda self: self.flipped_i32 != 0)
    candidate = property(lambda self: self.candidate_i32 != 0)


@dataclass
class PrecomputedSearch:
    """What `grade_precomputed_frames` returns: device tensors, one row per candidate frame, laid out as `LocalSearch`
    lays them out (`ints` (B, F, L, T, 6), `scores` (B, F, L, T), `slab_count` (B, F, L), `valid_index` (B, F), `count`
    (B,)); the named fields are views."""
    ints: torch.Tensor
    scores: torch.Tensor
    slab_count: torch.Tensor
    valid_i32: torch.Tensor
    valid_index: torch.Tensor
    count: torch.Tensor
    points: torch.Tensor
    frames: torch.Tensor
    config: PrecomputedViewConfig
    unbatched: bool = False

    search_score = property(lambda self: self.ints[..., 0])
    objects_label = property(lambda self: self.ints[..., 1])
    back = property(lambda self: self.ints[..., 2])
    finger = property(lambda self: self.ints[..., 3])
    close = property(lambda self: self.ints[..., 4])
    table_collision = property(lambda self: self.ints[..., 5])
    antipodal_score = property(lambda self: self.scores)
    valid = property(lambda self: self.valid_i32 != 0)

    def frames_of(self, index=None):
        """The reference's `valid_frame` (:388-394) of the rows `index` (B, K) (default: `valid_index`): (B, K, L, T, 4,
        4) = [R | p] @ LOCAL_SEARCH_TO_LOCAL, formed directly as `LocalSearch.frames_of` forms it (no `torch.inverse`,
        :124).  Rows whose index is -1 are 0."""
        return LocalSearch.frames_of(self._as_local(), index)

    def _as_local(self):
        return LocalSearch(self.ints, self.scores, self.slab_count, self.valid_i32, self.valid_index, self.count,
                           self.points, self.frames, self.config.search, self.unbatched)


@dataclass
class PrecomputedViewLabels:
    """What `label_precomputed_view` returns: `match` (`PrecomputedMatch`, per view point), `search`
    (`PrecomputedSearch`, row f = the candidate `match.frame_index[:, f]`) and `cloud_index` (B, F) int32: the view
    points of the valid frames in ascending order, then -1 -- what the reference's `valid_index` stores (:395)."""
    match: PrecomputedMatch
    search: PrecomputedSearch
    cloud_index: torch.Tensor

    def dump(self, b=0):
        """The dictionary of the reference's `dump()` (:249-254) for scene b, in the WORLD frame (the camera transform
        is the caller's, as for `LocalSearch.dump` and `ContactLabels.dump`).  Reads the count on the host."""
        s = self.search
        n = int(s.count[b])
        vi = s.valid_index[b, :n].long()
        L, T = s.config.search.shape
        return {"search_score": s.search_score[b, vi].cpu().numpy(),
                "antipodal_score": s.antipodal_score[b, vi].cpu().numpy(),
                "objects_label": s.objects_label[b, vi].to(torch.int16).cpu().numpy(),
                "point_cloud": self.match.cloud[b].cpu().numpy(),
                "valid_index": self.cloud_index[b, :n].cpu().numpy(),
                "valid_frame": s.frames_of(s.valid_index[b:b + 1, :n])[0].cpu().numpy()
                if n else torch.zeros((0, L, T, 4, 4)).numpy()}


def _batched_scene(scene):
    """A `DarbouxScene` (one scene: a leading 1 is added) or any object with its nine fields carrying a leading batch
    dimension -> dict of contiguous device tensors: points, normals (B, 3, M) fp32, labels (B, M) int32, frames (B, M,
    3, 3) fp32, the four scores (B, M, L, T)."""
    got = {}
    for name in _SCENE_FIELDS:
        t = getattr(scene, name, None)
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("scene.%s must be a CUDA tensor (there is no CPU fallback)" % name)
        got[name] = t
    if got["points"].dim() == 2:
        got = {k: v[None] for k, v in got.items()}
    pts = got["points"]
    if pts.dim() != 3 or pts.size(1) != 3 or pts.size(2) < 1:
        raise RuntimeError("scene.points must be (B, 3, M) with M >= 1")
    B, _, M = pts.shape
    ss = got["search_score"]
    if ss.dim() != 4 or ss.size(0) != B or ss.size(1) != M:
        raise RuntimeError("scene.search_score must be (B, M, L, T)")
    L, T = int(ss.size(2)), int(ss.size(3))
    want = {"points": (B, 3, M), "normals": (B, 3, M), "labels": (B, M), "frames": (B, M, 3, 3),
            "inv_frames": (B, M, 3, 3)}
    for name in _SCENE_FIELDS:
        shape = want.get(name, (B, M, L, T))
        if tuple(got[name].shape) != shape:
            raise RuntimeError("scene.%s must be %s, got %s" % (name, shape, tuple(got[name].shape)))
    if len({t.device for t in got.values()}) != 1:
        raise RuntimeError("every field of the scene must live on one device")
    if got["labels"].dtype != torch.int32:
        raise RuntimeError("scene.labels must be int32, got %s" % got["labels"].dtype)
    for name in ("search_score", "inv_search_score"):
        if got[name].dtype != torch.int32:
            raise RuntimeError("scene.%s must be int32, got %s" % (name, got[name].dtype))
    out = {k: v.contiguous() for k, v in got.items()}
    for name in ("points", "normals", "frames", "antipodal_score", "inv_antipodal_score"):
        out[name] = _F._f32c(out[name], "scene." + name)
    return out, B, M, L, T


def _check_lt(cfg, L, T):
    cfg.search.check()
    if not (1 <= L <= LS_MAX_DEPTHS and 1 <= T <= LS_MAX_ANGLES):
        raise ValueError("need 1..%d depths and 1..%d angles, got %d and %d" % (LS_MAX_DEPTHS, LS_MAX_ANGLES, L, T))
    if (L, T) != cfg.search.shape:
        raise ValueError("the scores hold %d x %d placements, config.search %d x %d" % ((L, T) + cfg.search.shape))


def match_scene_frames(reference_cloud, cloud, scene, camera, config=None, radius=CURVATURE_RADIUS):
    """`TorchPrecomputedSingleViewPointCloud._find_match` with `magic_formula` (:130-185) for every view point of every
    scene in one sync-free, graph-capturable call -> `PrecomputedMatch`.

    reference_cloud (B, 3, N) the noise-free view points the match runs on (`reference_cloud[index_in_ref]`); cloud
    (B, 3, N) the noisy view; scene a `DarbouxScene` or an object with its nine fields and a leading batch dimension
    (the scenes of a batch share M; pad with NaN points, which are never a neighbour); camera (B, 3) or (3,) the camera
    location.  One unbatched view (3, N) gets a leading 1.  Per view point: i = `match_nearest` on reference_cloud; the
    normal of i, or (0, 0, 1) without one, normalised in double, turned towards the camera seen from the NOISY point,
    rounded once; flipped where n . frame[:, 0] > 0 in double (:163); the scene frame of i with columns 0 and 1
    negated where flipped (:166; `inv_frames` is not read); the scene's scores, the inv_* ones where flipped
    (:167-170); mask = pre_search > search_threshold and pre_antipodal > antipodal_threshold, both compared in double
    as numpy does (:181-183); a candidate where matched, some mask bit is set and the noisy z > sample_region in fp32
    (:172-174).  An unmatched or non-finite view point keeps the identity frame and zero scores and is no candidate."""
    cfg = config or PrecomputedViewConfig()
    cfg.search.check()
    for name, t in (("reference_cloud", reference_cloud), ("cloud", cloud), ("camera", camera)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    sc, B, M, L, T = _batched_scene(scene)
    _check_lt(cfg, L, T)
    unbatched = cloud.dim() == 2
    if unbatched:
        reference_cloud, cloud = reference_cloud[None], cloud[None]
    ref = _F._f32c(reference_cloud, "reference_cloud")
    xyz = _F._f32c(cloud, "cloud")
    if xyz.dim() != 3 or xyz.size(1) != 3 or xyz.size(0) != B:
        raise RuntimeError("cloud must be (B, 3, N) with the scene's B")
    N = xyz.size(2)
    if tuple(ref.shape) != (B, 3, N):
        raise RuntimeError("reference_cloud must be (B, 3, N) like cloud")
    cam = _F._f32c(camera, "camera")
    if cam.dim() == 1 and cam.numel() == 3:
        cam = cam.view(1, 3).expand(B, 3)
    if tuple(cam.shape) != (B, 3):
        raise RuntimeError("camera must be (B, 3) or (3,)")
    cam = cam.contiguous()
    dev = xyz.device
    if len({ref.device, dev, cam.device, sc["points"].device}) != 1:
        raise RuntimeError("every input must live on one device")
    nearest = match_nearest(ref, sc["points"], radius)
    normals = torch.empty((B, 3, N), dtype=torch.float32, device=dev)
    flipped = torch.empty((B, N), dtype=torch.int32, device=dev)
    frames = torch.empty((B, N, 3, 3), dtype=torch.float32, device=dev)
    pre_search = torch.empty((B, N, L, T), dtype=torch.int32, device=dev)
    pre_antipodal = torch.empty((B, N, L, T), dtype=torch.float32, device=dev)
    mask = torch.empty((B, N, L, T), dtype=torch.bool, device=dev)
    candidate = torch.empty((B, N), dtype=torch.int32, device=dev)
    frame_index = torch.empty((B, N), dtype=torch.int32, device=dev)
    frame_count = torch.empty((B,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_precomputed_select_f32(
            nearest.data_ptr(), xyz.data_ptr(), sc["normals"].data_ptr(), cam.data_ptr(), sc["frames"].data_ptr(),
            sc["search_score"].data_ptr(), sc["inv_search_score"].data_ptr(), sc["antipodal_score"].data_ptr(),
            sc["inv_antipodal_score"].data_ptr(), B, N, M, L, T,
            float("-inf") if cfg.search_threshold is None else float(cfg.search_threshold),
            float(cfg.antipodal_threshold), float(cfg.region), normals.data_ptr(), flipped.data_ptr(),
            frames.data_ptr(), pre_search.data_ptr(), pre_antipodal.data_ptr(), mask.data_ptr(), candidate.data_ptr(),
            frame_index.data_ptr(), frame_count.data_ptr(), _F._stream())
    _cabi.check(rc, "precomputed_select")
    return PrecomputedMatch(nearest, normals, flipped, frames, pre_search, pre_antipodal, mask, candidate, frame_index,
                            frame_count, xyz, cfg, unbatched)


def grade_precomputed_frames(points, frames, mask, pre_search, pre_antipodal, scene_points, scene_labels, config=None,
                             frame_count=None):
    """`TorchPrecomputedSingleViewPointCloud.finger_hand` with `_table_collision_check` (:258-396), which `run_score`
    (:232-235) loops over the candidate frames, for F rows per scene in one sync-free, graph-capturable call ->
    `PrecomputedSearch`.

    points (B, F, 3) the noisy view points and frames (B, F, 3, 3) (axes as columns); mask (B, F, L, T) bool,
    pre_search (B, F, L, T) int32 and pre_antipodal (B, F, L, T) fp32 as `match_scene_frames` gives them; scene_points
    (B, 3, M) fp32 and scene_labels (B, M) int32 the dense scene (a NaN point is in no region); frame_count (B,) on the
    device (optional): only the first frame_count[b] rows of scene b are frames.  Unbatched inputs get a leading 1.
    Only placements whose mask bit is set are collision-checked; one that passes every gate (:327-371) takes over
    pre_search and pre_antipodal and the close region's label, every other one reads 0 / 0 / no_label.  The only frame
    gate is mean |frame| < 1e-6 (:295): `grade_local_search`'s reach gate does not exist in this class.  No stale
    slots, as for `grade_local_search`; `frames_of` is formed directly."""
    cfg = config or PrecomputedViewConfig()
    cfg.search.check()
    for name, t in (("points", points), ("frames", frames), ("mask", mask), ("pre_search", pre_search),
                    ("pre_antipodal", pre_antipodal), ("scene_labels", scene_labels)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    unbatched = points.dim() == 2
    if unbatched:
        points, frames, mask = points[None], frames[None], mask[None]
        pre_search, pre_antipodal = pre_search[None], pre_antipodal[None]
        scene_points, scene_labels = scene_points[None], scene_labels[None]
    xyz, _, lab, B, M, dev = _dense_scene(scene_points, scene_labels, same_device=[
        ("points", points), ("frames", frames), ("mask", mask), ("pre_search", pre_search),
        ("pre_antipodal", pre_antipodal)], size="M", nonempty=True)
    if mask.dim() != 4 or mask.size(0) != B:
        raise RuntimeError("mask must be (B, F, L, T)")
    F, L, T = int(mask.size(1)), int(mask.size(2)), int(mask.size(3))
    _check_lt(cfg, L, T)
    if points.dtype != torch.float32 or frames.dtype != torch.float32 or pre_antipodal.dtype != torch.float32:
        raise RuntimeError("points, frames and pre_antipodal must be float32")
    if mask.dtype != torch.bool or pre_search.dtype != torch.int32:
        raise RuntimeError("mask must be bool and pre_search int32")
    if tuple(points.shape) != (B, F, 3) or tuple(frames.shape) != (B, F, 3, 3):
        raise RuntimeError("points must be (B, F, 3) and frames (B, F, 3, 3)")
    if tuple(pre_search.shape) != (B, F, L, T) or tuple(pre_antipodal.shape) != (B, F, L, T):
        raise RuntimeError("pre_search and pre_antipodal must be (B, F, L, T) like mask")
    pts, frm, msk = points.contiguous(), frames.contiguous(), mask.contiguous()
    ps, pa = pre_search.contiguous(), pre_antipodal.contiguous()
    cnt = _scene_count(frame_count, B, dev, "frame_count")
    s = cfg.search
    tb = s.tables()
    tables = _small_on_device(torch.cat([tb["depth"], tb["lo"], tb["hi"], tb["cos"], tb["sin"]]), torch.float32, dev)
    ints = torch.empty((B, F, L, T, 6), dtype=torch.int32, device=dev)
    scores = torch.empty((B, F, L, T), dtype=torch.float32, device=dev)
    slab = torch.empty((B, F, L), dtype=torch.int32, device=dev)
    valid = torch.empty((B, F), dtype=torch.int32, device=dev)
    valid_index = torch.empty((B, F), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int64, device=dev)
    params = (ctypes.c_float * 13)(s.finger_length, s.bottom_length, s.half_hand_thickness, s.half_bottom_width,
                                   s.half_bottom_space, s.back_collision_margin, s.back_collision_threshold,
                                   s.finger_collision_threshold, s.close_region_min_points,
                                   s.table_height + s.table_collision_offset, s.num_points_threshold,
                                   cfg.valid_search_min, cfg.valid_antipodal_min)
    ws, nbytes = _workspace(_cabi.lib().s4g_precomputed_search_workspace_bytes(B, M, F, L, T), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_precomputed_search_f32(
            pts.data_ptr(), frm.data_ptr(), msk.data_ptr(), ps.data_ptr(), pa.data_ptr(), xyz.data_ptr(),
            lab.data_ptr(), B, M, F, L, T, params, int(s.no_label), tables.data_ptr(),
            None if cnt is None else cnt.data_ptr(), ints.data_ptr(), scores.data_ptr(), slab.data_ptr(),
            valid.data_ptr(), valid_index.data_ptr(), count.data_ptr(), ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "precomputed_search")
    return PrecomputedSearch(ints, scores, slab, valid, valid_index, count, pts, frm, cfg, unbatched)


def label_precomputed_view(reference_cloud, cloud, scene, camera, config=None, radius=CURVATURE_RADIUS):
    """`TorchPrecomputedSingleViewPointCloud.run_score` (:219-235): view cloud and `DarbouxScene` in, S4G labels out, in
    one sync-free, graph-capturable call -> `PrecomputedViewLabels`.  `match_scene_frames`, a gather of the candidate
    rows on the device (F = N rows, `frame_count` of them live, as `label_view` pads), then
    `grade_precomputed_frames`; see both for the arguments and the decisions.  A view without candidates has
    `frame_count` 0 (the reference stops in a debugger there)."""
    cfg = config or PrecomputedViewConfig()
    m = match_scene_frames(reference_cloud, cloud, scene, camera, cfg, radius)
    sc = _batched_scene(scene)[0]
    B, N = m.frame_index.shape
    L, T = m.mask.shape[2:]
    g = m.frame_index.clamp(min=0).to(torch.int64)
    rows = lambda t, width: torch.gather(t.reshape(B, N, width), 1, g.view(B, N, 1).expand(B, N, width))
    points = rows(m.cloud.transpose(1, 2), 3)
    frames = rows(m.frames, 9).view(B, N, 3, 3)
    mask = rows(m.mask, L * T).view(B, N, L, T)
    pre_search = rows(m.pre_search, L * T).view(B, N, L, T)
    pre_antipodal = rows(m.pre_antipodal, L * T).view(B, N, L, T)
    s = grade_precomputed_frames(points, frames, mask, pre_search, pre_antipodal, sc["points"], sc["labels"], cfg,
                                 m.frame_count)
    return PrecomputedViewLabels(m, s, map_cloud_index(s.valid_index, m.frame_index))


CR_MAX_RESOLUTION = 64                     # the compiled maximum of csrc/close_region.hip
CR_DEFAULT_POINTS_PER_FRAME = 4096         # the default capacity is F * min(N, this)


@dataclass
class ProjectionConfig:
    """PROJECTION_RESOLUTION and PROJECTION_MARGIN (data_gen/configs/config.py:93-94).  The box the maps cover comes from
    the gripper constants (torch_baseline_single_view_point_cloud.py:11-13): x = FINGER_LENGTH, y = 2 * HALF_BOTTOM_SPACE,
    z = 2 * HALF_HAND_THICKNESS."""
    resolution: int = 60
    margin: int = 1

    def check(self):
        if not (2 <= int(self.resolution) <= CR_MAX_RESOLUTION):
            raise ValueError("resolution must be 2..%d, got %r" % (CR_MAX_RESOLUTION, self.resolution))
        if not (0 <= self.margin < self.resolution):
            raise ValueError("margin must be in [0, resolution)")

    @staticmethod
    def dims(gripper=None):
        g = gripper or LocalSearchConfig()
        return (g.finger_length, g.half_bottom_space * 2, g.half_hand_thickness * 2)

    def units(self, gripper=None):
        """dim / (resolution - margin) per axis in Python floats (:16-18), rounded to fp32 once."""
        return tuple(float(torch.tensor(d / (self.resolution - self.margin), dtype=torch.float32))
                     for d in self.dims(gripper))

    def heights(self, gripper=None):
        """(h0, hstep) per axis, fp32 values: the height of voxel k is h0 + k * hstep =
        torch.linspace(unit / 2, dim - unit / 2, resolution)[k] (:379-381), which is (k + 0.5) * unit when margin is 0."""
        out = []
        for d in self.dims(gripper):
            u = d / (self.resolution - self.margin)
            out.append((float(torch.tensor(0.5 * u, dtype=torch.float32)),
                        float(torch.tensor((d - u) / (self.resolution - 1), dtype=torch.float32))))
        return tuple(out)


@dataclass
class BestPlacement:
    """What `best_placement` returns: `index` (B, F) int32 (-1 where the frame is invalid), `score` (B, F),
    `global_to_local` (B, F, 4, 4) (the reference's `baseline_frame`, 0 where invalid), `valid_index` (B, F) ascending
    and -1 padded, `count` (B,) int64."""
    index: torch.Tensor
    score: torch.Tensor
    global_to_local: torch.Tensor
    valid_index: torch.Tensor
    count: torch.Tensor
    unbatched: bool = False

    valid = property(lambda self: self.index >= 0)


def best_placement(search):
    """The fold of `TorchBaseLineSingleViewPointCloud.finger_hand` (torch_baseline_single_view_point_cloud.py:308-312,
    323-331) over a `LocalSearch`: per frame, over the L * T placements in flattened order, the first one whose
    antipodal score is > 0 and > every earlier score (a NaN is never taken); the frame is valid unless that score is
    < 1e-4.  -> `BestPlacement`; `global_to_local` = LOCAL_TO_LOCAL_SEARCH[index] @ [R^T | -R^T p], formed directly in fp32."""
    if not isinstance(search, LocalSearch):
        raise RuntimeError("best_placement takes the LocalSearch that grade_local_search returns")
    scores = search.scores
    if scores.device.type != "cuda":
        raise RuntimeError("search must hold CUDA tensors (there is no CPU fallback)")
    dev = scores.device
    B, F, L, T = scores.shape
    tb = search.config.tables()
    tables = _small_on_device(torch.cat([tb["depth"], tb["lo"], tb["hi"], tb["cos"], tb["sin"]]), torch.float32, dev)
    index = torch.empty((B, F), dtype=torch.int32, device=dev)
    score = torch.empty((B, F), dtype=torch.float32, device=dev)
    g2l = torch.empty((B, F, 4, 4), dtype=torch.float32, device=dev)
    valid_index = torch.empty((B, F), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int64, device=dev)
    sc = scores.contiguous()
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_best_placement_f32(search.points.data_ptr(), search.frames.data_ptr(), sc.data_ptr(),
                                                tables.data_ptr(), B, F, L, T, index.data_ptr(), score.data_ptr(),
                                                g2l.data_ptr(), valid_index.data_ptr(), count.data_ptr(), _F._stream())
    _cabi.check(rc, "best_placement")
    return BestPlacement(index, score, g2l, valid_index, count, search.unbatched)


@dataclass
class CloseRegions:
    """What `close_regions` returns.  `count` (B, F) int32, `offset` (B, F + 1) int64, `points` / `normals`
    (B, 3, capacity), `index` (B, capacity) int32, `maps` (B, F, 12, R, R), `flags` (B, F) int32 (bit 0: the set does
    not fit; bit 1: a kept point or normal is not finite).  Frame f's set is the slice offset[f]:offset[f + 1]."""
    count: torch.Tensor
    offset: torch.Tensor
    points: torch.Tensor
    normals: torch.Tensor
    index: torch.Tensor
    maps: torch.Tensor
    flags: torch.Tensor
    unbatched: bool = False

    def sets(self, b=0, frames=None):
        """The lists of the reference's `dump()` (:195-197) for the frames `frames` of scene b (default: every frame
        with flags 0): (close_region_points_set, close_region_normals_set, close_region_projection_map_set) as lists of
        numpy arrays (3, n), (3, n), (12, R, R).  Reads the counts on the host."""
        off = self.offset[b].cpu().tolist()
        fl = self.flags[b].cpu().tolist()
        if frames is None:
            frames = [f for f in range(len(fl)) if fl[f] == 0]
        P, Nn, M = self.points[b].cpu().numpy(), self.normals[b].cpu().numpy(), self.maps[b].cpu().numpy()
        frames = [int(f) for f in frames]
        keep = [(off[f], off[f + 1]) if not (fl[f] & 1) else (0, 0) for f in frames]
        return ([P[:, lo:hi].copy() for lo, hi in keep], [Nn[:, lo:hi].copy() for lo, hi in keep],
                [M[f].copy() for f in frames])


def close_regions(global_to_local, cloud, normals, gripper=None, x_range=None, live=None, frame_count=None,
                  capacity=None, projection=None):
    """The crop and `close_region_projection` of the baselines' data generators
    (torch_baseline_single_view_point_cloud.py:294-318,334-393; torch_precomputed_baseline.py:350-383) for every frame
    of every scene in one sync-free, graph-capturable call -> `CloseRegions`.

    global_to_local (B, F, 4, 4) fp32 (`BestPlacement.global_to_local`); cloud, normals (B, 3, N) fp32; unbatched inputs
    get a leading 1.  Rows with live == 0 (live (B, F), optional) or at or past frame_count[b] (optional) are not
    scanned: count 0, flags 0, zero maps.  A point is in the region iff x_lo < lx < x_hi, |ly| < half_bottom_space and
    |lz| < half_hand_thickness, every inequality strict, the bounds rounded to fp32 once.  x_range defaults to
    (-bottom_length, finger_length), the baseline class, whose depth slab is the only x filter; (0, finger_length) is
    the precomputed class's box.  `gripper` is any object with finger_length, bottom_length, half_bottom_space and
    half_hand_thickness (default `LocalSearchConfig()`); `projection` a `ProjectionConfig`.  capacity (points per scene
    in the packed buffers) defaults to F * min(N, 4096) and must be below 2^31; `count` and `offset` are exact whatever
    it is, a frame whose set does not fit is flagged and not stored.  Normal components are clamped to [-4, 4] in the
    maps' voxel sums (fixed point, as the band sums of `grade_local_search`)."""
    g = gripper or LocalSearchConfig()
    proj = projection or ProjectionConfig()
    proj.check()
    for name, t in (("global_to_local", global_to_local), ("cloud", cloud), ("normals", normals)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
        if t.dtype != torch.float32:
            raise RuntimeError("%s must be float32" % name)
    unbatched = global_to_local.dim() == 3
    if unbatched:
        global_to_local, cloud, normals = global_to_local[None], cloud[None], normals[None]
        live = None if live is None else live[None]
    if cloud.dim() != 3 or cloud.size(1) != 3 or cloud.size(2) < 1:
        raise RuntimeError("cloud must be (B, 3, N)")
    B, _, N = cloud.shape
    if tuple(normals.shape) != (B, 3, N):
        raise RuntimeError("normals must be (B, 3, N) like cloud")
    if global_to_local.dim() != 4 or global_to_local.size(0) != B or tuple(global_to_local.shape[2:]) != (4, 4):
        raise RuntimeError("global_to_local must be (B, F, 4, 4)")
    if len({global_to_local.device, cloud.device, normals.device}) != 1:
        raise RuntimeError("global_to_local, cloud and normals must live on one device")
    dev = cloud.device
    F = global_to_local.shape[1]
    if live is not None:
        if not isinstance(live, torch.Tensor) or live.device != dev or tuple(live.shape) != (B, F):
            raise RuntimeError("live must be a (B, F) tensor on the device of cloud")
        live = live.to(torch.int32).contiguous()
    cnt = _scene_count(frame_count, B, dev, "frame_count")
    capacity = F * min(N, CR_DEFAULT_POINTS_PER_FRAME) if capacity is None else int(capacity)
    if not (0 <= capacity < 2 ** 31):
        raise ValueError("capacity must be in [0, 2^31), got %d" % capacity)
    x_lo, x_hi = (-g.bottom_length, g.finger_length) if x_range is None else x_range
    units, heights = proj.units(g), proj.heights(g)
    params = (ctypes.c_float * 13)(x_lo, x_hi, g.half_bottom_space, g.half_hand_thickness, *units,
                                   *[h[0] for h in heights], *[h[1] for h in heights])
    R = int(proj.resolution)
    G, xyz, nrm = global_to_local.contiguous(), cloud.contiguous(), normals.contiguous()
    count = torch.empty((B, F), dtype=torch.int32, device=dev)
    offset = torch.empty((B, F + 1), dtype=torch.int64, device=dev)
    points = torch.empty((B, 3, capacity), dtype=torch.float32, device=dev)
    out_n = torch.empty((B, 3, capacity), dtype=torch.float32, device=dev)
    index = torch.empty((B, capacity), dtype=torch.int32, device=dev)
    maps = torch.empty((B, F, 12, R, R), dtype=torch.float32, device=dev)
    flags = torch.empty((B, F), dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(_cabi.lib().s4g_close_region_workspace_bytes(B, N, F, capacity), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_close_region_f32(G.data_ptr(), xyz.data_ptr(), nrm.data_ptr(),
                                              None if live is None else live.data_ptr(),
                                              None if cnt is None else cnt.data_ptr(), B, N, F, capacity, R, params,
                                              count.data_ptr(), offset.data_ptr(), points.data_ptr(), out_n.data_ptr(),
                                              index.data_ptr(), maps.data_ptr(), flags.data_ptr(), ws.data_ptr(), nbytes,
                                              _F._stream())
    _cabi.check(rc, "close_region")
    return CloseRegions(count, offset, points, out_n, index, maps, flags, unbatched)


@dataclass
class BaselineLabels:
    """What `label_baseline_view` returns: the `LocalSearch` (without the label gate), its `BestPlacement` and the
    `CloseRegions` of the best placements."""
    search: LocalSearch
    best: BestPlacement
    regions: CloseRegions

    def dump(self, b=0):
        """The dictionary of the reference's `dump()` (torch_baseline_single_view_point_cloud.py:189-198) for scene b, in
        the world frame (the camera transform is the caller's); `point_cloud` holds the frame origins (3, F).  Reads the
        counts on the host."""
        n = int(self.best.count[b])
        vi = self.best.valid_index[b, :n].long()
        pts, nrm, maps = self.regions.sets(b, vi.cpu().tolist())
        return {"antipodal_score": self.best.score[b, vi].cpu().numpy(),
                "point_cloud": self.search.points[b].t().contiguous().cpu().numpy(),
                "valid_index": vi.int().cpu().numpy(),
                "baseline_frame": self.best.global_to_local[b, vi].cpu().numpy(),
                "close_region_points_set": pts, "close_region_normals_set": nrm,
                "close_region_projection_map_set": maps}


def label_baseline_view(points, frames, scene_points, scene_normals, cloud=None, normals=None, config=None,
                        projection=None, frame_count=None, x_range=None, capacity=None, camera=None):
    """`run_score` of `TorchBaseLineSingleViewPointCloud` (torch_baseline_single_view_point_cloud.py:158-181,220-331) as
    one sync-free call -> `BaselineLabels`: `grade_local_search` with one label for every scene point (which removes
    the label gate, the only difference between the two searches), `best_placement`, then `close_regions` of `cloud` /
    `normals` (default: the scene itself, as in that class) in the best placement of every valid frame.  The
    reference's stop after `grasp_num` valid frames is the caller's slice of `best.valid_index`; no stale slots, as in
    `grade_local_search`.  `TorchPrecomputedBaselinePointCloud`, which looks its scores up in a precomputed scene, is
    `label_precomputed_baseline_view`.

    camera (B, 3) or (3,), the camera location: a cloud without normals gets them from `estimate_normals(cloud,
    camera)` with the reference's radius and max_nn, as that class does for a cloud that has none (:69-70): `cloud`
    may then come with normals=None, and scene_normals=None with cloud=None estimates the scene's.  Without `camera`
    nothing is estimated and cloud and normals go together, as before."""
    cfg = config or LocalSearchConfig()
    if not isinstance(scene_points, torch.Tensor) or scene_points.device.type != "cuda":
        raise RuntimeError("scene_points must be a CUDA tensor (there is no CPU fallback)")
    if camera is None:
        if (cloud is None) != (normals is None):
            raise RuntimeError("cloud and normals go together")
    else:
        if cloud is None and normals is not None:
            raise RuntimeError("cloud and normals go together")
        if scene_normals is None:
            if cloud is not None:
                raise RuntimeError("scene_normals=None estimates the normals of the scene as the cloud: pass cloud=None")
            est = estimate_normals(scene_points, camera)
            scene_normals = est.normals[0] if est.unbatched else est.normals
        elif cloud is not None and normals is None:
            est = estimate_normals(cloud, camera)
            normals = est.normals[0] if est.unbatched else est.normals
    lab_shape = scene_points.shape[:-2] + scene_points.shape[-1:]
    labels = torch.zeros(lab_shape, dtype=torch.int32, device=scene_points.device)
    search = grade_local_search(points, frames, scene_points, scene_normals, labels, cfg, frame_count)
    best = best_placement(search)
    if cloud is None:
        cloud, normals = scene_points, scene_normals
    if search.unbatched and cloud.dim() == 2:
        cloud, normals = cloud[None], normals[None]
    regions = close_regions(best.global_to_local, cloud, normals, cfg, x_range, best.index >= 0, frame_count, capacity,
                            projection)
    regions.unbatched = search.unbatched
    return BaselineLabels(search, best, regions)


@dataclass
class PrecomputedBaselineConfig:
    """The constants of the fast baseline labels (torch_precomputed_baseline.py): the threshold of `magic_formula`
    (:178), SAMPLE_REGION (None: table_height + SAMPLE_REGION_OFFSET of `search`), the local search's own constants and
    the projection maps'."""
    antipodal_threshold: float = 0.3
    sample_region: float = None
    search: LocalSearchConfig = None
    projection: ProjectionConfig = None

    def __post_init__(self):
        if self.search is None:
            self.search = LocalSearchConfig()
        if self.projection is None:
            self.projection = ProjectionConfig()

    def view_config(self):
        """The `PrecomputedViewConfig` that makes `match_scene_frames` this class's `_find_match`: the search
        threshold switched off."""
        return PrecomputedViewConfig(search_threshold=None, antipodal_threshold=self.antipodal_threshold,
                                     sample_region=self.sample_region, search=self.search)


@dataclass
class PrecomputedBaselineSearch:
    """What `grade_precomputed_baseline_frames` returns: device tensors, one row per candidate frame.  `ints`
    (B, F, L, T, 4) int32 = back, finger, close, table verdict; `scores` (B, F, L, T) the looked-up score where every gate
    passed, else 0; `slab_count` (B, F, L); `points`, `frames` as given; `best` the `BestPlacement` of the fold."""
    ints: torch.Tensor
    scores: torch.Tensor
    slab_count: torch.Tensor
    points: torch.Tensor
    frames: torch.Tensor
    best: BestPlacement
    config: PrecomputedBaselineConfig
    unbatched: bool = False

    back = property(lambda self: self.ints[..., 0])
    finger = property(lambda self: self.ints[..., 1])
    close = property(lambda self: self.ints[..., 2])
    table_collision = property(lambda self: self.ints[..., 3])
    antipodal_score = property(lambda self: self.scores)


def grade_precomputed_baseline_frames(points, frames, mask, pre_antipodal, scene_points, config=None, frame_count=None):
    """`TorchPrecomputedBaselinePointCloud.finger_hand` with `_table_collision_check`
    (torch_precomputed_baseline.py:227-348, 381-382), which `run_score` (:193-199) loops over the candidate frames, for
    F rows per scene in one sync-free, graph-capturable call -> `PrecomputedBaselineSearch`.

    points (B, F, 3) the noisy view points and frames (B, F, 3, 3) (axes as columns); mask (B, F, L, T) bool and
    pre_antipodal (B, F, L, T) fp32 as `match_scene_frames` gives them with the search threshold off; scene_points
    (B, 3, M) fp32 the dense scene (a NaN point is in no region); frame_count (B,) on the device (optional).  Unbatched
    inputs get a leading 1.  Only placements whose mask bit is set are collision-checked, with the counts of
    `grade_precomputed_frames` bit for bit; there is no label gate, so a close region on two objects passes.  `best`
    is the reference's fold (:337-348): the first placement, depths outer and rolls inner, that passes every gate and
    whose looked-up score is > 0 and > every earlier taken one; `best.global_to_local` =
    LOCAL_TO_LOCAL_SEARCH[index] @ [R^T | -R^T p] (:381-382), formed directly.  No stale slots."""
    cfg = config or PrecomputedBaselineConfig()
    cfg.search.check()
    for name, t in (("points", points), ("frames", frames), ("mask", mask), ("pre_antipodal", pre_antipodal),
                    ("scene_points", scene_points)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    unbatched = points.dim() == 2
    if unbatched:
        points, frames, mask, pre_antipodal = points[None], frames[None], mask[None], pre_antipodal[None]
        scene_points = scene_points[None]
    xyz = _F._f32c(scene_points, "scene_points")
    if xyz.dim() != 3 or xyz.size(1) != 3 or xyz.size(2) < 1:
        raise RuntimeError("scene_points must be (B, 3, M) with M >= 1")
    B, _, M = xyz.shape
    dev = xyz.device
    if len({dev, points.device, frames.device, mask.device, pre_antipodal.device}) != 1:
        raise RuntimeError("every input must live on one device")
    if mask.dim() != 4 or mask.size(0) != B:
        raise RuntimeError("mask must be (B, F, L, T)")
    F, L, T = int(mask.size(1)), int(mask.size(2)), int(mask.size(3))
    _check_lt(cfg, L, T)
    if points.dtype != torch.float32 or frames.dtype != torch.float32 or pre_antipodal.dtype != torch.float32:
        raise RuntimeError("points, frames and pre_antipodal must be float32")
    if mask.dtype != torch.bool:
        raise RuntimeError("mask must be bool")
    if tuple(points.shape) != (B, F, 3) or tuple(frames.shape) != (B, F, 3, 3):
        raise RuntimeError("points must be (B, F, 3) and frames (B, F, 3, 3)")
    if tuple(pre_antipodal.shape) != (B, F, L, T):
        raise RuntimeError("pre_antipodal must be (B, F, L, T) like mask")
    pts, frm, msk, pa = points.contiguous(), frames.contiguous(), mask.contiguous(), pre_antipodal.contiguous()
    cnt = _scene_count(frame_count, B, dev, "frame_count")
    s = cfg.search
    tb = s.tables()
    tables = _small_on_device(torch.cat([tb["depth"], tb["lo"], tb["hi"], tb["cos"], tb["sin"]]), torch.float32, dev)
    ints = torch.empty((B, F, L, T, 4), dtype=torch.int32, device=dev)
    scores = torch.empty((B, F, L, T), dtype=torch.float32, device=dev)
    slab = torch.empty((B, F, L), dtype=torch.int32, device=dev)
    index = torch.empty((B, F), dtype=torch.int32, device=dev)
    score = torch.empty((B, F), dtype=torch.float32, device=dev)
    g2l = torch.empty((B, F, 4, 4), dtype=torch.float32, device=dev)
    valid_index = torch.empty((B, F), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int64, device=dev)
    params = (ctypes.c_float * 11)(s.finger_length, s.bottom_length, s.half_hand_thickness, s.half_bottom_width,
                                   s.half_bottom_space, s.back_collision_margin, s.back_collision_threshold,
                                   s.finger_collision_threshold, s.close_region_min_points,
                                   s.table_height + s.table_collision_offset, s.num_points_threshold)
    ws, nbytes = _workspace(_cabi.lib().s4g_precomputed_baseline_search_workspace_bytes(B, M, F, L, T), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_precomputed_baseline_search_f32(
            pts.data_ptr(), frm.data_ptr(), msk.data_ptr(), pa.data_ptr(), xyz.data_ptr(), B, M, F, L, T, params,
            tables.data_ptr(), None if cnt is None else cnt.data_ptr(), ints.data_ptr(), scores.data_ptr(),
            slab.data_ptr(), index.data_ptr(), score.data_ptr(), g2l.data_ptr(), valid_index.data_ptr(),
            count.data_ptr(), ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "precomputed_baseline_search")
    best = BestPlacement(index, score, g2l, valid_index, count, unbatched)
    return PrecomputedBaselineSearch(ints, scores, slab, pts, frm, best, cfg, unbatched)


@dataclass
class PrecomputedBaselineLabels:
    """What `label_precomputed_baseline_view` returns: `match` (`PrecomputedMatch`, per view point), `search`
    (`PrecomputedBaselineSearch`, row f = the candidate `match.frame_index[:, f]`; `best` = `search.best`), `regions`
    (`CloseRegions` of the VIEW cloud in the best placement of every valid frame) and `cloud_index` (B, F) int32: the
    view points of the valid frames in ascending order, then -1 -- what the reference's `valid_index` stores (:377)."""
    match: PrecomputedMatch
    search: PrecomputedBaselineSearch
    regions: CloseRegions
    cloud_index: torch.Tensor

    best = property(lambda self: self.search.best)

    def dump(self, b=0, grasp_num=None):
        """The dictionary of the reference's `dump()` (:216-223) for scene b, in the WORLD frame; grasp_num: the
        reference's stop after that many valid frames.  `baseline_frame` is `se3_inverse(global_to_local)` (local
        search -> world): the reference stores that matrix times the inverse camera pose, and the camera transform is
        the caller's, as everywhere else.  `point_cloud` is the whole noisy view (3, N), `valid_index` holds the
        view-point indices.  Reads the count on the host."""
        best = self.search.best
        n = int(best.count[b])
        if grasp_num is not None:
            n = min(n, int(grasp_num))
        vi = best.valid_index[b, :n].long()
        pts, nrm, maps = self.regions.sets(b, vi.cpu().tolist())
        return {"antipodal_score": best.score[b, vi].cpu().numpy(),
                "point_cloud": self.match.cloud[b].cpu().numpy(),
                "valid_index": self.cloud_index[b, :n].cpu().numpy(),
                "close_region_points_set": pts, "close_region_normals_set": nrm,
                "close_region_projection_map_set": maps,
                "baseline_frame": se3_inverse(best.global_to_local[b, vi]).cpu().numpy()}


def label_precomputed_baseline_view(reference_cloud, cloud, scene, camera, config=None, radius=CURVATURE_RADIUS,
                                    capacity=None):
    """`TorchPrecomputedBaselinePointCloud.run_score` (torch_precomputed_baseline.py:182-204): view cloud and
    `DarbouxScene` in, the inputs GPD and PointNetGPD are trained and evaluated on out, in one sync-free,
    graph-capturable call -> `PrecomputedBaselineLabels`.  `match_scene_frames` with the search threshold off (the
    mask is pre_antipodal > antipodal_threshold alone, compared in double; the scene's `search_score` fields are carried
    but not read for the mask), the gather of the candidate rows on the device as `label_precomputed_view` does it,
    `grade_precomputed_baseline_frames`, then `close_regions` of the VIEW cloud with the matched and oriented normals in
    the best placement of every valid frame, x in (0, finger_length) (:350-383).  An unmatched or non-finite view point
    is never a candidate but stays in the crop's cloud with its (0, 0, 1)-towards-camera normal, as the reference has
    it.  A frame whose best placement has an empty view crop is valid with `regions.count` 0 (the reference appends an
    empty set).  The reference's stop after `grasp_num` valid frames is the caller's slice of `best.valid_index`; no
    stale slots; `local_to_global` is never formed by `torch.inverse`."""
    cfg = config or PrecomputedBaselineConfig()
    m = match_scene_frames(reference_cloud, cloud, scene, camera, cfg.view_config(), radius)
    sc = _batched_scene(scene)[0]
    B, N = m.frame_index.shape
    L, T = m.mask.shape[2:]
    g = m.frame_index.clamp(min=0).to(torch.int64)
    rows = lambda t, width: torch.gather(t.reshape(B, N, width), 1, g.view(B, N, 1).expand(B, N, width))
    points = rows(m.cloud.transpose(1, 2), 3)
    frames = rows(m.frames, 9).view(B, N, 3, 3)
    mask = rows(m.mask, L * T).view(B, N, L, T)
    pre_antipodal = rows(m.pre_antipodal, L * T).view(B, N, L, T)
    s = grade_precomputed_baseline_frames(points, frames, mask, pre_antipodal, sc["points"], cfg, m.frame_count)
    best = s.best
    s.unbatched = best.unbatched = m.unbatched
    s4 = cfg.search
    regions = close_regions(best.global_to_local, m.cloud, m.normals, s4, (0, s4.finger_length), best.index >= 0,
                            m.frame_count, capacity, cfg.projection)
    regions.unbatched = m.unbatched
    return PrecomputedBaselineLabels(m, s, regions, map_cloud_index(best.valid_index, m.frame_index))


def _regions_and_best(labels_or_regions, who):
    if isinstance(labels_or_regions, (BaselineLabels, PrecomputedBaselineLabels, EvalViewLabels)):
        return labels_or_regions.regions, labels_or_regions.best
    if isinstance(labels_or_regions, CloseRegions):
        return labels_or_regions, None
    raise RuntimeError("%s takes the BaselineLabels of label_baseline_view, the PrecomputedBaselineLabels of "
                       "label_precomputed_baseline_view, the EvalViewLabels of label_eval_view or their CloseRegions" % who)


def score_projections(labels_or_regions, runner, grasp_num=None):
    """The GPD baseline's classifier on the maps of `label_baseline_view` or `label_precomputed_baseline_view`, still on the device and without a gathered
    copy: `runner` (a `baselines.FusedGPD`) reads `regions.maps` in place through
    `best.valid_index[:, :grasp_num]` -> logits (B, K, classes), K = min(grasp_num, F); rows at or past `best.count[b]`
    are zero.  The reference's stop after `grasp_num` valid frames is the slice.  Given `CloseRegions` alone, every
    frame is scored -> (B, F, classes)."""
    regions, best = _regions_and_best(labels_or_regions, "score_projections")
    if not callable(runner):
        raise RuntimeError("runner must be a baselines.FusedGPD")
    if best is None:
        if grasp_num is not None:
            raise RuntimeError("grasp_num needs the BaselineLabels (the valid frames are in its best placement)")
        return runner(regions.maps)
    index = best.valid_index
    if grasp_num is not None:
        if int(grasp_num) < 0:
            raise ValueError("grasp_num must be >= 0, got %r" % (grasp_num,))
        index = index[:, :int(grasp_num)]
    return runner(regions.maps, index=index)


def score_close_regions(labels_or_regions, runner, grasp_num=None):
    """The PointNetGPD baseline's classifier on the point sets of `label_baseline_view` or `label_precomputed_baseline_view`, still on the device and without
    a gathered or sampled copy: `runner` (a `baselines.FusedPointNetGPD`) reads `regions.points` in place through
    `offset` / `count` / `flags` and `best.valid_index[:, :grasp_num]`, every set whole and at its true size -> logits
    (B, K, classes), K = min(grasp_num, F); rows at or past `best.count[b]` are zero, and so is the row of a frame whose
    set is empty or did not fit the capacity.  Given `CloseRegions` alone, every frame is scored -> (B, F, classes)."""
    regions, best = _regions_and_best(labels_or_regions, "score_close_regions")
    if not callable(runner):
        raise RuntimeError("runner must be a baselines.FusedPointNetGPD")
    if best is None:
        if grasp_num is not None:
            raise RuntimeError("grasp_num needs the BaselineLabels (the valid frames are in its best placement)")
        return runner(regions.points, offset=regions.offset, count=regions.count, flags=regions.flags)
    index = best.valid_index
    if grasp_num is not None:
        if int(grasp_num) < 0:
            raise ValueError("grasp_num must be >= 0, got %r" % (grasp_num,))
        index = index[:, :int(grasp_num)]
    return runner(regions.points, offset=regions.offset, count=regions.count, flags=regions.flags, index=index)


@dataclass
class EvalDataConfig:
    """The constants of the baselines' evaluation data (data_gen/eval/evaluation_data_generator.py): the local search's
    own (`search`), `grasp_num` (:33, :61), the sample region (None: table_height + SAMPLE_REGION_OFFSET - 0.02 of
    `search`, :59) and the neighbour minimum of a frame (:145)."""
    search: LocalSearchConfig = None
    grasp_num: int = 2000
    sample_region: float = None
    min_neighbours: int = 5

    def __post_init__(self):
        if self.search is None:
            self.search = LocalSearchConfig()

    def region(self):
        if self.sample_region is not None:
            return float(self.sample_region)
        return self.search.table_height + SAMPLE_REGION_OFFSET - 0.02


@dataclass
class EvalViewSearch:
    """What `grade_eval_view_frames` returns: device tensors, one row per frame.  `ints` (B, F, L, T, 4) int32 = back,
    finger, close, table verdict; `slab_count` (B, F, L); `index` (B, F) int32 the FIRST passing placement or -1;
    `global_to_local` (B, F, 4, 4) the reference's `baseline_frame`, 0 where invalid; `flags` (B, F) int32 (1 not
    scanned, 2 not finite, 4 frame gate, 8 reach gate); `valid_index` (B, F) ascending and -1 padded; `count` (B,)
    int64; `points`, `frames` as given."""
    ints: torch.Tensor
    slab_count: torch.Tensor
    index: torch.Tensor
    global_to_local: torch.Tensor
    flags: torch.Tensor
    valid_index: torch.Tensor
    count: torch.Tensor
    points: torch.Tensor
    frames: torch.Tensor
    config: EvalDataConfig
    unbatched: bool = False

    back = property(lambda self: self.ints[..., 0])
    finger = property(lambda self: self.ints[..., 1])
    close = property(lambda self: self.ints[..., 2])
    table_collision = property(lambda self: self.ints[..., 3])
    valid = property(lambda self: self.index >= 0)


@dataclass
class EvalSceneGrades:
    """What `grade_eval_scene_frames` returns: device tensors, one row per pose.  `ints` (B, K, 8) int32 = slab, back,
    finger, close, more than one label, n_left, n_right, stage; `non_collision`, `single_label` (B, K) uint8, as the
    reference stores them; `antipodal_score` (B, K) fp32; `floats` (B, K, 4) = left_y, right_y, mean_left, mean_right.
    `stage` is the line at which the reference returned: 0 scored, 1 slab, 2 back, 3 finger, 4 labels, 5 few points
    (`ints[..., 7]` holds 16 more for a pose that is not finite: `not_finite`)."""
    ints: torch.Tensor
    non_collision: torch.Tensor
    single_label: torch.Tensor
    antipodal_score: torch.Tensor
    floats: torch.Tensor

    slab = property(lambda self: self.ints[..., 0])
    back = property(lambda self: self.ints[..., 1])
    finger = property(lambda self: self.ints[..., 2])
    close = property(lambda self: self.ints[..., 3])
    multi_objects = property(lambda self: self.ints[..., 4] != 0)
    n_left = property(lambda self: self.ints[..., 5])
    n_right = property(lambda self: self.ints[..., 6])
    stage = property(lambda self: self.ints[..., 7] & 15)
    not_finite = property(lambda self: (self.ints[..., 7] & 16) != 0)
    left_y = property(lambda self: self.floats[..., 0])
    right_y = property(lambda self: self.floats[..., 1])
    mean_left = property(lambda self: self.floats[..., 2])
    mean_right = property(lambda self: self.floats[..., 3])


def _live_rows(live, shape, device, name):
    """The optional row list `live` (B, rows), any dtype -> int32 on the device (0 = not scanned), or None."""
    if live is None:
        return None
    if not isinstance(live, torch.Tensor) or live.device != device or tuple(live.shape) != tuple(shape):
        raise RuntimeError("%s must be a %s tensor on the device of the cloud" % (name, tuple(shape)))
    return (live != 0).to(torch.int32).contiguous()


def grade_eval_view_frames(points, frames, cloud, config=None, frame_count=None, live=None):
    """`EvalDataGenerator.finger_hand_view` with `_table_collision_check` (evaluation_data_generator.py:209-330), which
    `run_collision` (:199-200) loops over the sampled frames, for F frames of each of B views in one sync-free,
    graph-capturable call -> `EvalViewSearch`.

    points (B, F, 3) frame origins, frames (B, F, 3, 3) (axes as columns), cloud (B, 3, N) fp32 the VIEW cloud the
    placements are checked against (a point that is not finite is in no region); unbatched inputs get a leading 1.
    frame_count (B,) on the device (optional): rows at or past it are not scanned; live (B, F) (optional): rows that read
    0 are not scanned -- `label_eval_view` passes the frames with enough neighbours, whose frame the reference leaves at
    zero.  Per frame the frame gate, the reach gate, then depths outer and rolls inner the FIRST placement whose depth
    slab is populated, whose box clears the table, and whose back, finger and close counts pass; there is no score, no
    label gate and no best.  The counts are those of `grade_precomputed_baseline_frames` with an all-true mask, bit for
    bit.  No stale slots: a row that is not taken reads index -1 and a zero matrix."""
    cfg = config or EvalDataConfig()
    s = cfg.search
    s.check()
    for name, t in (("points", points), ("frames", frames), ("cloud", cloud)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    unbatched = points.dim() == 2
    if unbatched:
        points, frames, cloud = points[None], frames[None], cloud[None]
        live = None if live is None else live[None]
    xyz = _F._f32c(cloud, "cloud")
    if xyz.dim() != 3 or xyz.size(1) != 3 or xyz.size(2) < 1:
        raise RuntimeError("cloud must be (B, 3, N) with N >= 1")
    B, _, N = xyz.shape
    dev = xyz.device
    if len({dev, points.device, frames.device}) != 1:
        raise RuntimeError("points, frames and cloud must live on one device")
    if points.dtype != torch.float32 or frames.dtype != torch.float32:
        raise RuntimeError("points and frames must be float32")
    if points.dim() != 3 or points.size(0) != B or points.size(2) != 3:
        raise RuntimeError("points must be (B, F, 3)")
    F = points.shape[1]
    if tuple(frames.shape) != (B, F, 3, 3):
        raise RuntimeError("frames must be (B, F, 3, 3)")
    pts, frm = points.contiguous(), frames.contiguous()
    cnt = _scene_count(frame_count, B, dev, "frame_count")
    lv = _live_rows(live, (B, F), dev, "live")
    L, T = s.shape
    tb = s.tables()
    tables = _small_on_device(torch.cat([tb["depth"], tb["lo"], tb["hi"], tb["cos"], tb["sin"]]), torch.float32, dev)
    ints = torch.empty((B, F, L, T, 4), dtype=torch.int32, device=dev)
    slab = torch.empty((B, F, L), dtype=torch.int32, device=dev)
    index = torch.empty((B, F), dtype=torch.int32, device=dev)
    g2l = torch.empty((B, F, 4, 4), dtype=torch.float32, device=dev)
    flags = torch.empty((B, F), dtype=torch.int32, device=dev)
    valid_index = torch.empty((B, F), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int64, device=dev)
    params = (ctypes.c_float * 12)(s.finger_length, s.bottom_length, s.half_hand_thickness, s.half_bottom_width,
                                   s.half_bottom_space, s.back_collision_margin, s.back_collision_threshold,
                                   s.finger_collision_threshold, s.close_region_min_points,
                                   s.table_height + s.table_collision_offset, s.num_points_threshold, s.table_height)
    ws, nbytes = _workspace(_cabi.lib().s4g_eval_view_search_workspace_bytes(B, N, F, L, T), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_eval_view_search_f32(
            pts.data_ptr(), frm.data_ptr(), xyz.data_ptr(), B, N, F, L, T, params, tables.data_ptr(),
            None if cnt is None else cnt.data_ptr(), None if lv is None else lv.data_ptr(), ints.data_ptr(),
            slab.data_ptr(), index.data_ptr(), g2l.data_ptr(), flags.data_ptr(), valid_index.data_ptr(),
            count.data_ptr(), ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "eval_view_search")
    return EvalViewSearch(ints, slab, index, g2l, flags, valid_index, count, pts, frm, cfg, unbatched)


def grade_eval_scene_frames(global_to_local, scene_points, scene_normals, scene_labels, config=None, count=None,
                            live=None):
    """`EvalDataGenerator.finger_hand_scene` with `_antipodal_score` (evaluation_data_generator.py:161-186,332-391),
    which `run_collision` (:205-206) loops over the valid grasps, for K poses of each of B scenes in one sync-free,
    graph-capturable call -> `EvalSceneGrades`.

    global_to_local (B, K, 4, 4) fp32 (`EvalViewSearch.global_to_local`, the reference's `baseline_frame`);
    scene_points, scene_normals (B, 3, M) fp32; scene_labels (B, M) int32.  count (B,) on the device (optional): rows at
    or past it are not scanned; live (B, K) (optional): rows that read 0 are not scanned; such rows read 0 everywhere.
    The transform, the regions, the label test, the bands and the score are `eval_frames`' bit for bit wherever both
    reach the score; this class adds the slab count and returns in its own order (`stage`).  An EMPTY close region has
    a single label, as written."""
    cfg = config or EvalDataConfig()
    s = cfg.search
    if not isinstance(global_to_local, torch.Tensor) or global_to_local.device.type != "cuda":
        raise RuntimeError("global_to_local must be a CUDA tensor (there is no CPU fallback)")
    if global_to_local.dtype != torch.float32:
        raise RuntimeError("global_to_local must be float32")
    if global_to_local.dim() == 3:
        global_to_local = global_to_local[None]
        scene_points, scene_normals, scene_labels = scene_points[None], scene_normals[None], scene_labels[None]
        live = None if live is None else live[None]
    xyz, nrm, lab, B, M, dev = _dense_scene(scene_points, scene_labels, scene_normals,
                                            [("global_to_local", global_to_local)], size="M", nonempty=True)
    if global_to_local.dim() != 4 or global_to_local.size(0) != B or tuple(global_to_local.shape[2:]) != (4, 4):
        raise RuntimeError("global_to_local must be (B, K, 4, 4)")
    K = global_to_local.shape[1]
    g2l = global_to_local.contiguous()
    cnt = _scene_count(count, B, dev, "count")
    lv = _live_rows(live, (B, K), dev, "live")
    ints = torch.empty((B, K, 8), dtype=torch.int32, device=dev)
    non_collision = torch.empty((B, K), dtype=torch.uint8, device=dev)
    single_label = torch.empty((B, K), dtype=torch.uint8, device=dev)
    score = torch.empty((B, K), dtype=torch.float32, device=dev)
    floats = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
    params = (ctypes.c_float * 11)(s.finger_length, s.bottom_length, s.half_hand_thickness, s.half_bottom_width,
                                   s.half_bottom_space, s.back_collision_margin, s.back_collision_threshold,
                                   s.finger_collision_threshold, s.close_region_min_points, s.neighbor_depth,
                                   s.num_points_threshold)
    ws, nbytes = _workspace(_cabi.lib().s4g_eval_scene_grade_workspace_bytes(B, M, K), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_eval_scene_grade_f32(
            g2l.data_ptr(), xyz.data_ptr(), nrm.data_ptr(), lab.data_ptr(), B, M, K, params,
            None if cnt is None else cnt.data_ptr(), None if lv is None else lv.data_ptr(), ints.data_ptr(),
            non_collision.data_ptr(), single_label.data_ptr(), score.data_ptr(), floats.data_ptr(), ws.data_ptr(),
            nbytes, _F._stream())
    _cabi.check(rc, "eval_scene_grade")
    return EvalSceneGrades(ints, non_collision, single_label, score, floats)


@dataclass
class EvalViewLabels:
    """What `label_eval_view` returns: `frames` (`DarbouxFrames` of the sampled view points), `search`
    (`EvalViewSearch`, row f = frame f), `regions` (`CloseRegions` of the VIEW cloud in the placement taken) and `truth`
    (`EvalSceneGrades` of the taken placements against the dense scene; a row without one reads 0).  `cloud`, `normals`
    are the view as it was searched; the scene tensors are kept for `dump`."""
    frames: DarbouxFrames
    search: EvalViewSearch
    regions: CloseRegions
    truth: EvalSceneGrades
    cloud: torch.Tensor
    normals: torch.Tensor
    scene_points: torch.Tensor
    scene_normals: torch.Tensor
    scene_labels: torch.Tensor

    best = property(lambda self: self.search)     # (what `score_projections` / `score_close_regions` read: valid_index)

    def dump(self, b=0):
        """The dictionary of the reference's `dump()` (evaluation_data_generator.py:96-107) for view b in the WORLD
        frame (the camera transform is the caller's), the grasps in the reference's append order, which is ascending
        frame.  `frame` is `se3_inverse(global_to_local)`, the rigid inverse formed directly where the reference calls
        `torch.inverse`.  Reads the count on the host."""
        n = int(self.search.count[b])
        vi = self.search.valid_index[b, :n].long()
        pts, nrm, maps = self.regions.sets(b, vi.cpu().tolist())
        return {"frame": se3_inverse(self.search.global_to_local[b, vi]).cpu().numpy(),
                "antipodal_score": self.truth.antipodal_score[b, vi].cpu().numpy(),
                "non_collision_bool": self.truth.non_collision[b, vi].cpu().numpy(),
                "single_label_bool": self.truth.single_label[b, vi].cpu().numpy(),
                "view_cloud": self.cloud[b].t().contiguous().cpu().numpy(),
                "scene_cloud": self.scene_points[b].t().contiguous().cpu().numpy(),
                "scene_label": self.scene_labels[b].cpu().numpy(),
                "scene_normal": self.scene_normals[b].t().contiguous().cpu().numpy(),
                "close_region_points_set": pts, "close_region_normals_set": nrm,
                "close_region_projection_map_set": maps}


def label_eval_view(cloud, normals, scene_points, scene_normals, scene_labels, config=None, frame_index=None,
                    frame_count=None, camera=None, projection=None, capacity=None, generator=None):
    """`EvalDataGenerator.run_collision` (data_gen/eval/evaluation_data_generator.py:188-207), what
    `generate_eval_data.py` runs per rendered view: rendered view and dense labelled scene in, the baselines'
    candidate grasps with their classifier inputs and their ground truth out, as one sync-free chain ->
    `EvalViewLabels`.

    cloud (B, 3, N) fp32 the processed view (`process_views`), normals like it or None with `camera` (B, 3) or (3,):
    `estimate_normals(cloud, camera)` (:65-66).  scene_points, scene_normals (B, 3, M) fp32, scene_labels (B, M) int32.
    Steps: `estimate_frames` at frame_index; `grade_eval_view_frames` of those frames against the VIEW with live =
    neighbour count >= config.min_neighbours; `close_regions` of the view in the placement taken, x in (-bottom_length,
    finger_length) (the depth slab is this class's only x filter); `grade_eval_scene_frames` of the taken placements.

    frame_index (B, F) int32 with frame_count (B,), or None: the first config.grasp_num points with z >
    config.region() in ascending index (:59-61).  `generator` (a device torch.Generator) shuffles those candidates on
    the device first, as the reference's `np.random.shuffle` does; its unseeded order cannot be reproduced.

    Decisions.  (1) No stale slots.  (2) `dump()['frame']` is the rigid inverse formed directly.  (3) A point with
    fewer than min_neighbours neighbours is not a candidate: the reference leaves its frame at zero (:63, :145), which
    fails the frame gate, where `estimate_frames` returns the identity and reports `count`.  (4) The eigenvector sign
    is `estimate_frames`' pinned rule; the other sign maps roll theta to -theta and can change which placement is
    first.  (5) An empty scene close region has a single label, as written.  (6) The crop tests the composed matrix
    where the reference tests the unshifted slab: points within rounding of a face are ambiguous, as in
    `label_baseline_view`."""
    cfg = config or EvalDataConfig()
    if not isinstance(cloud, torch.Tensor) or cloud.device.type != "cuda":
        raise RuntimeError("cloud must be a CUDA tensor (there is no CPU fallback)")
    if cloud.dim() != 3:
        raise RuntimeError("cloud must be (B, 3, N)")
    if normals is None:
        if camera is None:
            raise RuntimeError("a cloud without normals needs the camera location")
        normals = estimate_normals(cloud, camera).normals
    xyz = _F._f32c(cloud, "cloud")
    B, _, N = xyz.shape
    if frame_index is None:
        if frame_count is not None:
            raise RuntimeError("frame_count needs a frame_index")
        index, cnt = sample_frame_index(xyz, cfg.region())
        if generator is not None:
            keys = torch.rand((B, N), generator=generator, device=xyz.device)
            pad = torch.arange(N, device=xyz.device).view(1, N) >= cnt.view(B, 1)
            index = torch.gather(index, 1, torch.argsort(keys.masked_fill(pad, 2.0), dim=1))
        F = min(int(cfg.grasp_num), N)
        frame_index, frame_count = index[:, :F].contiguous(), cnt.clamp(max=F)
    fr = estimate_frames(xyz, normals, frame_index, frame_count, min_neighbours=cfg.min_neighbours)
    search = grade_eval_view_frames(fr.points, fr.frames, xyz, cfg, fr.frame_count, fr.count >= cfg.min_neighbours)
    taken = search.index >= 0
    regions = close_regions(search.global_to_local, xyz, normals.contiguous(), cfg.search, None, taken, fr.frame_count,
                            capacity, projection)
    truth = grade_eval_scene_frames(search.global_to_local, scene_points, scene_normals, scene_labels, cfg,
                                    fr.frame_count, taken)
    return EvalViewLabels(fr, search, regions, truth, xyz, normals, scene_points, scene_normals, scene_labels)


from .contact_object import *  # noqa: E402,F401,F403  (the refine and reduce stages of the contact-object pipeline)
from .render import *  # noqa: E402,F401,F403  (the rendered views the view stage starts from)
