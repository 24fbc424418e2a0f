"""The refine and reduce stages of the contact-object pipeline: data_gen/utils/refine_contact_object.py and
data_gen/utils/smooth_contact_object.py of the reference, which stand between `label_contact_object` and
`compose_contact_scene`.  Host code only; the kernels are csrc/contact_refine.hip and s4g_match_knn_f32 of
csrc/match_normals.hip (contract: include/s4g_ops.h).  `postprocess` re-exports every public name of this module, and
this module reads `postprocess`'s host plumbing inside its calls (the two modules import each other)."""
import ctypes
from dataclasses import dataclass

import torch

from . import _cabi
from . import functions as _F

__all__ = ["ContactRefineConfig", "ContactReduceConfig", "ContactRefinement", "ContactReduction",
           "RefinedContactFrames", "refine_contact_frames", "reduce_contact_frames", "refine_contact_object",
           "reduce_contact_object", "REFINE_FAIL_FINGER", "REFINE_FAIL_FEW", "REFINE_FAIL_BEHIND",
           "REFINE_FAIL_NONFINITE", "REFINE_FAIL_FILTERED", "REDUCE_MAX_POINTS", "REDUCE_OVERFLOW"]

REFINE_FAIL_FINGER, REFINE_FAIL_FEW, REFINE_FAIL_BEHIND, REFINE_FAIL_NONFINITE, REFINE_FAIL_FILTERED = 1, 2, 4, 8, 16
REDUCE_MAX_POINTS = 65536                  # the fold's running counts are one byte of LDS per point
REDUCE_MAX_NN = 8
REDUCE_OVERFLOW = 1
_MAX_LIST = 4                              # the compiled maximum of each shift list (csrc/contact_refine.hip)


@dataclass
class ContactRefineConfig:
    """The constants of refine_contact_object.py:18-23 and the gripper of data_gen/configs/config.py:50-56.
    `post_process_single_grasp.py` is the same test with collision_threshold 3 and one placement."""
    height_search: tuple = (-0.01, 0.01, 0)
    width_search: tuple = (0,)
    length_search: tuple = (-0.01, 0.01, 0)
    min_search_score: int = 100
    collision_threshold: int = 0
    half_bottom_width: float = 0.057
    bottom_length: float = 0.08
    finger_width: float = 0.023
    half_hand_thickness: float = 0.012
    finger_length: float = 0.09

    @property
    def half_bottom_space(self):
        return self.half_bottom_width - self.finger_width

    @property
    def shape(self):
        """(nz, ny, nx); placement (iz * ny + iy) * nx + ix, the script's loop order (dz outer, dx inner)."""
        return len(self.height_search), len(self.width_search), len(self.length_search)

    @property
    def placements(self):
        nz, ny, nx = self.shape
        return nz * ny * nx

    def check(self):
        for name, n in zip(("height_search", "width_search", "length_search"), self.shape):
            if not 1 <= n <= _MAX_LIST:
                raise ValueError("%s needs 1..%d entries, got %d" % (name, _MAX_LIST, n))
        if int(self.min_search_score) != self.min_search_score or not 1 <= self.min_search_score < (1 << 24):
            raise ValueError("min_search_score must be an integer in [1, 2^24): with a minimum of 1 the count gate "
                             "precedes the minimum of an empty close region, where the script raises; got %r"
                             % (self.min_search_score,))
        if int(self.collision_threshold) != self.collision_threshold or self.collision_threshold < 0:
            raise ValueError("collision_threshold must be an integer >= 0, got %r" % (self.collision_threshold,))

    def tables(self):
        """The bounds of :75-85, formed in Python floats and rounded to fp32 once, in `ContactSearchConfig.tables`'
        layout: the sign of dy in `ylo` / `yhi` (+) and in |y + dy| is the script's."""
        from .postprocess import ContactSearchConfig
        return ContactSearchConfig(width_search=self.width_search, height_search=self.height_search,
                                   length_search=self.length_search, half_bottom_width=self.half_bottom_width,
                                   bottom_length=self.bottom_length, finger_width=self.finger_width,
                                   half_hand_thickness=self.half_hand_thickness,
                                   finger_length=self.finger_length).tables()


@dataclass
class ContactReduceConfig:
    """The constants of smooth_contact_object.py:14-16 and the literals of :71-72."""
    min_search_score: float = 50
    frame_per_point: int = 5
    max_neighbor_frame: int = 4
    min_rest: int = 5
    radius: float = 0.01
    max_nn: int = 5

    def check(self):
        if not 1 <= int(self.frame_per_point) <= 255:
            raise ValueError("frame_per_point must be in [1, 255] (the running counts are bytes), got %r"
                             % (self.frame_per_point,))
        if not 0 <= int(self.max_neighbor_frame) <= int(self.frame_per_point):
            raise ValueError("max_neighbor_frame must be in [0, frame_per_point], got %r" % (self.max_neighbor_frame,))
        if not 1 <= int(self.max_nn) <= REDUCE_MAX_NN:
            raise ValueError("max_nn must be in [1, %d], got %r" % (REDUCE_MAX_NN, self.max_nn))
        if int(self.min_rest) < int(self.max_nn) - 1:
            raise ValueError("min_rest must be at least max_nn - 1 (every neighbour rank then has a frame of the rest), "
                             "got %r with max_nn %r" % (self.min_rest, self.max_nn))
        if not float(self.radius) > 0.0:
            raise ValueError("radius must be positive, got %r" % (self.radius,))


@dataclass
class ContactRefinement:
    """What `refine_contact_frames` returns, one row per frame: `counts` (B, F, P, 3) int32 = {finger, close, behind} per
    placement, `kept_i32`, `fail` (B, F) int32 (the REFINE_FAIL_* bits), `search_score` (B, F) fp32 the minimum close
    count of a kept frame (an exact integer) and 0 elsewhere, `kept_index` (B, F) int32 the kept rows ascending then
    -1, `kept_count` (B,) int64."""
    counts: torch.Tensor
    kept_i32: torch.Tensor
    search_score: torch.Tensor
    fail: torch.Tensor
    kept_index: torch.Tensor
    kept_count: torch.Tensor
    config: ContactRefineConfig
    unbatched: bool = False

    finger = property(lambda self: self.counts[..., 0])
    close = property(lambda self: self.counts[..., 1])
    behind = property(lambda self: self.counts[..., 2])
    kept = property(lambda self: self.kept_i32 != 0)


@dataclass
class ContactReduction:
    """What `reduce_contact_frames` returns: `source_frame`, `point_index` (B, cap) int32 in the script's append order,
    -1 past `count` (B,) int64, which stays exact when the list did not fit (`flags` (B,) int32 & REDUCE_OVERFLOW);
    `neighbours` (B, N, max_nn) int32 the searched lists."""
    source_frame: torch.Tensor
    point_index: torch.Tensor
    count: torch.Tensor
    flags: torch.Tensor
    neighbours: torch.Tensor
    config: ContactReduceConfig
    unbatched: bool = False


@dataclass
class RefinedContactFrames:
    """The frames of every object after a stage, with the attributes `compose_contact_scene` reads of an
    `ObjectContactFrames`.  `search_score` is fp32 on the device and holds exact integers; `stage` is the
    `ContactRefinement` or `ContactReduction` behind the rows."""
    global_to_local: torch.Tensor
    search_score: torch.Tensor
    antipodal_score: torch.Tensor
    frame_point_index: torch.Tensor
    frame_count: torch.Tensor
    flags: torch.Tensor
    points: torch.Tensor
    normals: torch.Tensor
    count: torch.Tensor
    stage: object = None
    unbatched: bool = False

    def dump(self, b=0):
        """The dictionary the scripts pickle (refine_contact_object.py:112-114) for object b, as numpy with their
        dtypes: `search_score` and `frame_point_index` int64.  Reads the counts on the host."""
        n = self.points.shape[2] if self.count is None else int(self.count[b])
        f = min(int(self.frame_count[b]), self.global_to_local.shape[1])
        return {"cloud": self.points[b, :, :n].t().cpu().numpy(),
                "normal": self.normals[b, :, :n].t().cpu().numpy(),
                "global_to_local": self.global_to_local[b, :f].cpu().numpy(),
                "search_score": self.search_score[b, :f].to(torch.int64).cpu().numpy(),
                "antipodal_score": self.antipodal_score[b, :f].cpu().numpy(),
                "frame_point_index": self.frame_point_index[b, :f].to(torch.int64).cpu().numpy()}


def _frame_rows(t, name, B, dtype, dev, unbatched, tail=()):
    """A per-frame input (B, F) + tail on the device of the points; an unbatched call's gets a leading 1."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)
    if unbatched:
        t = t[None]
    if t.device != dev:
        raise RuntimeError("%s must live on the device of points" % name)
    if t.dim() != 2 + len(tail) or t.size(0) != B or tuple(t.shape[2:]) != tuple(tail):
        raise RuntimeError("%s must be (B, F%s)" % (name, "".join(", %d" % v for v in tail)))
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t.contiguous()


def refine_contact_frames(points, global_to_local, search_score, config=None, count=None, frame_count=None):
    """`check_single_collision` of data_gen/utils/refine_contact_object.py (:45-114) for every frame of every object in
    one sync-free, graph-capturable call on the library's stream -> `ContactRefinement`.

    points (B, 3, N) fp32 the object clouds; global_to_local (B, F, 4, 4) fp32; search_score (B, F) fp32; one unbatched
    object gets a leading 1.  count, frame_count (B,) on the device (optional): the points / rows of object b are its
    first count[b] / frame_count[b].  A row is scanned when search_score > min_search_score (:46); it is kept when under
    every placement (heights x widths x lengths, dz outer, dx inner) at most collision_threshold points lie in the
    fingers, at least min_search_score in the close region and none of those behind x = 0.  The new score is the
    smallest close count (:95).

    Decisions.  (1) min_search_score >= 1, so that the count gate precedes the minimum of an empty close region, where
    the script raises; `if search_result:` then never drops a kept frame.  (2) The script's early return means "any
    placement fails": all placements are counted.  (3) `check_single_collision(j)` reads the enclosing `i`; the loop
    passes `i`.  (4) A frame with an entry that is not finite is dropped (REFINE_FAIL_NONFINITE)."""
    from . import postprocess as P
    cfg = config or ContactRefineConfig()
    cfg.check()
    xyz, _, cnt, unbatched = P._object_cloud(points, None, count)
    B, _, N = xyz.shape
    dev = xyz.device
    g2l = _frame_rows(global_to_local, "global_to_local", B, torch.float32, dev, unbatched, (4, 4))
    F = g2l.shape[1]
    search = _frame_rows(search_score, "search_score", B, torch.float32, dev, unbatched)
    if search.shape[1] != F:
        raise RuntimeError("search_score must be (B, F) like global_to_local")
    if unbatched and isinstance(frame_count, torch.Tensor) and frame_count.dim() == 0:
        frame_count = frame_count[None]
    fcnt = P._scene_count(frame_count, B, dev, "frame_count")
    nz, ny, nx = cfg.shape
    npl = cfg.placements
    tb = cfg.tables()
    tables = P._small_on_device(torch.cat([tb[k] for k in ("zlo", "zhi", "ylo", "yhi", "dy", "xlo", "xhi")]),
                                torch.float32, dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)            # noqa: E731
    out = ContactRefinement(i32(B, F, npl, 3), i32(B, F), torch.empty((B, F), dtype=torch.float32, device=dev),
                            i32(B, F), i32(B, F), torch.empty((B,), dtype=torch.int64, device=dev), cfg, unbatched)
    params = (ctypes.c_float * 8)(cfg.finger_length, cfg.bottom_length, cfg.half_hand_thickness,
                                  cfg.half_bottom_width, cfg.half_bottom_space,
                                  max(abs(float(v)) for v in cfg.length_search),
                                  max(abs(float(v)) for v in cfg.width_search),
                                  max(abs(float(v)) for v in cfg.height_search))
    ws, nbytes = P._workspace(_cabi.lib().s4g_contact_refine_workspace_bytes(B, N, F, npl), dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()             # noqa: E731
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_contact_refine_f32(
            ptr(g2l), xyz.data_ptr(), ptr(search), B, N, F, nz, ny, nx, params, int(cfg.min_search_score),
            int(cfg.collision_threshold), tables.data_ptr(), ptr(cnt), ptr(fcnt), ptr(out.counts), ptr(out.kept_i32),
            ptr(out.search_score), ptr(out.fail), ptr(out.kept_index), out.kept_count.data_ptr(), ws.data_ptr(),
            nbytes, _F._stream())
    _cabi.check(rc, "contact_refine")
    return out


def reduce_contact_frames(points, frame_point_index, search_score, config=None, count=None, frame_count=None,
                          max_frames=None):
    """The fold of data_gen/utils/smooth_contact_object.py (:36-97) for every object in one sync-free, graph-capturable
    call on the library's stream -> `ContactReduction`: at most frame_per_point frames stay on a point, and a point
    with more than frame_per_point + min_rest hands one frame each to its max_nn nearest points within radius, as far
    as their own counts allow.

    points (B, 3, N) fp32, N <= 65 536 (the fold keeps one byte of LDS per point; refused above); frame_point_index
    (B, F) int; search_score (B, F) fp32; count, frame_count (B,) on the device (optional).  Frames may come in any
    point order; an index outside [0, count) counts for nobody.  The output holds rows of the list as given, in the
    script's append order; `point_index` of a spread frame is the neighbour's.  max_frames: the rows of the output
    (default min(F, N * frame_per_point)); `count` stays exact and `flags` says when it did not fit.

    Decision.  The neighbours come in the library's pinned order, (fp32 squared distance, index): a lower-index copy of
    point i ranks before i itself; open3d's order among equal distances is open."""
    from . import postprocess as P
    cfg = config or ContactReduceConfig()
    cfg.check()
    xyz, _, cnt, unbatched = P._object_cloud(points, None, count)
    B, _, N = xyz.shape
    dev = xyz.device
    if N > REDUCE_MAX_POINTS:
        raise ValueError("reduce_contact_frames serves at most %d points per object, got %d" % (REDUCE_MAX_POINTS, N))
    fpi = _frame_rows(frame_point_index, "frame_point_index", B, None, dev, unbatched)
    if fpi.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("frame_point_index must be int32 or int64, got %s" % fpi.dtype)
    F = fpi.shape[1]
    search = _frame_rows(search_score, "search_score", B, torch.float32, dev, unbatched)
    if search.shape[1] != F:
        raise RuntimeError("search_score must be (B, F) like frame_point_index")
    if unbatched and isinstance(frame_count, torch.Tensor) and frame_count.dim() == 0:
        frame_count = frame_count[None]
    fcnt = P._scene_count(frame_count, B, dev, "frame_count")
    cap = min(F, N * int(cfg.frame_per_point)) if max_frames is None else int(max_frames)
    if cap < 0:
        raise ValueError("max_frames must not be negative")
    fpi32, offsets, order = _frames_of_points(fpi, search, cfg, N, cnt, fcnt)
    knn = _neighbours(xyz, cnt, cfg)
    return _fold(fpi32, offsets, order, knn, cnt, cfg, cap, unbatched)


def _frames_of_points(fpi, search, cfg, N, cnt, fcnt):
    """(a) The frames of every point in ascending frame order, of the filtered list (:37, :62): a frame that fails the
    filter, or whose point is not one of the object's, sorts behind every point -> (frame_point_index with -1 on those
    frames, `frames_by_point`'s offsets and order)."""
    from . import postprocess as P
    lim = N if cnt is None else cnt.view(-1, 1)
    dead = ~(search > float(cfg.min_search_score)) | (fpi < 0) | (fpi >= lim)
    fpi32 = torch.where(dead, fpi.new_full((), -1), fpi).to(torch.int32).contiguous()
    offsets, order = P.frames_by_point(fpi32, N, fcnt)
    return fpi32, offsets, order


def _neighbours(xyz, cnt, cfg):
    """(b) The max_nn nearest points of every point within the radius (s4g_match_knn_f32) -> (B, N, max_nn) int32."""
    from . import postprocess as P
    B, _, N = xyz.shape
    dev = xyz.device
    live = None if cnt is None else cnt.clamp(0, N).to(torch.int32)
    knn = torch.empty((B, N, int(cfg.max_nn)), dtype=torch.int32, device=dev)
    ws, nbytes = P._workspace(_cabi.lib().s4g_estimate_normals_workspace_bytes(B, N), dev)
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_match_knn_f32(xyz.data_ptr(), None if live is None else live.data_ptr(), B, N,
                                           float(cfg.radius), int(cfg.max_nn), knn.data_ptr(), ws.data_ptr(), nbytes,
                                           _F._stream())
    _cabi.check(rc, "match_knn")
    return knn


def _fold(fpi32, offsets, order, knn, cnt, cfg, cap, unbatched=False):
    """(c) The fold (s4g_contact_reduce_i32) -> `ContactReduction`."""
    B, N = knn.shape[:2]
    F = fpi32.shape[1]
    dev = knn.device
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)            # noqa: E731
    out = ContactReduction(i32(B, cap), i32(B, cap), torch.empty((B,), dtype=torch.int64, device=dev), i32(B), knn, cfg,
                           unbatched)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()             # noqa: E731
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_contact_reduce_i32(
            ptr(fpi32), offsets.data_ptr(), ptr(order), knn.data_ptr(), ptr(cnt), B, N, F, int(cfg.frame_per_point),
            int(cfg.max_neighbor_frame), int(cfg.min_rest), int(cfg.max_nn), cap, ptr(out.source_frame),
            ptr(out.point_index), out.count.data_ptr(), out.flags.data_ptr(), _F._stream())
    _cabi.check(rc, "contact_reduce")
    return out


def _gather_rows(obj, rows):
    """The frames `rows` (B, K) int32 (-1 padded) of obj -> (global_to_local, antipodal_score, the int64 rows clamped to
    0, the padding mask); torch, no host read."""
    idx = rows.clamp(min=0).to(torch.int64)
    pad = rows < 0
    g2l = torch.gather(obj.global_to_local, 1, idx[:, :, None, None].expand(-1, -1, 4, 4))
    anti = torch.gather(obj.antipodal_score, 1, idx).masked_fill(pad, 0)
    return g2l, anti, idx, pad


def _batched(obj):
    """obj's per-frame tensors with a leading batch axis (an `ObjectContactFrames` always has one)."""
    if obj.global_to_local.dim() == 3:
        raise RuntimeError("the object's tensors must be batched (B, F, ...), as label_contact_object returns them")
    return obj


def refine_contact_object(obj, config=None):
    """The refine stage on what `label_contact_object` returned (an `ObjectContactFrames`, or anything with its
    attributes) -> `RefinedContactFrames`: `refine_contact_frames`, then `global_to_local`, `antipodal_score` and
    `frame_point_index` gathered through `kept_index` in torch, without a host read.  `search_score` is the new one;
    `frame_count` the kept count; the padded tail reads 0 / -1."""
    obj = _batched(obj)
    r = refine_contact_frames(obj.points, obj.global_to_local, obj.search_score, config, obj.count, obj.frame_count)
    g2l, anti, idx, pad = _gather_rows(obj, r.kept_index)
    score = torch.gather(r.search_score, 1, idx).masked_fill(pad, 0)
    fpi = torch.gather(obj.frame_point_index.to(torch.int32), 1, idx).masked_fill(pad, -1)
    return RefinedContactFrames(g2l, score, anti, fpi, r.kept_count, obj.flags, obj.points, obj.normals, obj.count, r,
                                getattr(obj, "unbatched", False))


def reduce_contact_object(obj, config=None):
    """The reduce stage on what `refine_contact_object` returned (or anything with its attributes) ->
    `RefinedContactFrames` in the script's append order, `frame_point_index` the point each frame now belongs to;
    `flags` gains REDUCE_OVERFLOW << 16 where the output did not fit, and `frame_count` is then the exact count, as
    everywhere."""
    obj = _batched(obj)
    search = obj.search_score.to(torch.float32)
    r = reduce_contact_frames(obj.points, obj.frame_point_index, search, config, obj.count, obj.frame_count)
    g2l, anti, idx, pad = _gather_rows(obj, r.source_frame)
    score = torch.gather(search, 1, idx).masked_fill(pad, 0)
    return RefinedContactFrames(g2l, score, anti, r.point_index, r.count, obj.flags | (r.flags << 16), obj.points,
                                obj.normals, obj.count, r, getattr(obj, "unbatched", False))
