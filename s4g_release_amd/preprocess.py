"""Cloud pre-processing on the HIP device ("next" row f3): the steps in front of the
network in the reference's `GraspDetector._pre_processing`
(grasp_proposal/grasp_detector.py:94-105) and `CloudPreProcessor`
(grasp_proposal/cloud_processor/cloud_processor.py:12-42).

Differences a maintainer should know:
  * the reference calls open3d's `voxel_down_sample` / `remove_radius_outlier` but
    drops the clouds they return (cloud_processor.py:34,40), so its network input is
    the raw cloud; here both steps APPLY (`CloudPreProcessor.points` is updated),
    which is what the config constants (processing_config.py:20-22) describe;
  * open3d emits voxels in hash-map order; here they come out in ascending
    (iz, iy, ix) cell order;
  * subsampling (`sample_single_cloud`, grasp_detector.py:82-92) is seeded
    (splitmix64-keyed permutation) or, as the reference's comment suggests, FPS.
Every step is a HIP kernel behind the C ABI (include/s4g_ops.h); there is no CPU path.

`process_views` is the batched, sync-free form of crop -> voxel -> outliers with the data GENERATOR's constants and
its trace (`processing_and_trace` of data_gen/pcd_classes/): the first stage of the label pipeline in postprocess.py.
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _cabi
from . import functions as _F

# processing_config.py:17-23
TABLE_HEIGHT = 0.75
WORKSPACE = (-0.40, 0.40, -0.4, 0.4, TABLE_HEIGHT - 0.001, TABLE_HEIGHT + 0.45)
VOXEL_SIZE = 0.005
NUM_POINTS_THRESHOLD = 32
RADIUS_THRESHOLD = 0.02
# grasp_detector.py:26
REAL2TRAIN = ((0., 1., 0., 0.), (1., 0., 0., 0.), (0., 0., -1., 0.), (0., 0., 0., 1.))


def _cloud(points):
    p = _F._f32c(points, "points")
    if p.dim() != 2 or p.size(0) != 3:
        raise RuntimeError("points must be (3, N)")
    return p


def filter_work_space(points, workspace=WORKSPACE):
    """Indices (ascending, int64) of the points strictly inside the workspace box."""
    p = _cloud(points)
    n = p.size(1)
    index = torch.empty(max(n, 1), dtype=torch.int32, device=p.device)
    count = torch.zeros(1, dtype=torch.int32, device=p.device)
    ws = (ctypes.c_float * 6)(*[float(v) for v in workspace])
    with torch.cuda.device(p.device):
        rc = _cabi.lib().s4g_crop_indices_f32(_F._ptr(p), n, ws, index.data_ptr(), count.data_ptr(),
                                              _F._stream())
    _cabi.check(rc, "crop_indices")
    return index[:int(count.item())].long()


def _voxel_grid(lo, hi, voxel):
    """(origin (3,) f32, dims (3,) int64) of the voxel grid over the bounds lo / hi (3,): origin = lo - voxel/2,
    dims = floor((hi - origin) / voxel) + 1, every operation in fp32 (oracle/preprocess.py voxel_grid).  Raises where
    the kernel would be handed a grid it cannot index: a NaN / inf bound, a dims value >= 2^31 (int32 in the C ABI),
    2^32 or more cells (uint32 keys)."""
    v = np.float32(voxel)
    lo = np.asarray(lo, dtype=np.float32)
    hi = np.asarray(hi, dtype=np.float32)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise RuntimeError("voxel_down_sample: non-finite coordinates in the cloud (NaN or inf), crop first")
    with np.errstate(over="ignore", invalid="ignore"):
        origin = (lo - v * np.float32(0.5)).astype(np.float32)
        top = np.floor(((hi - origin) / v).astype(np.float32))
    if not (np.isfinite(origin).all() and np.isfinite(top).all()) or (top >= 2.0 ** 31 - 1).any():
        raise RuntimeError("voxel grid too fine for this cloud (2^31 or more cells on one axis)")
    dims = top.astype(np.int64) + 1
    if int(dims[0]) * int(dims[1]) * int(dims[2]) >= 2 ** 32:
        raise RuntimeError("voxel grid too fine for this cloud (more than 2^32 cells)")
    return origin, dims


def voxel_down_sample(points, voxel_size=VOXEL_SIZE):
    """(3, V) voxel means (open3d VoxelDownSample semantics, cells in ascending order).  A cloud with a NaN or
    infinite coordinate has no grid: RuntimeError (crop first, `filter_work_space` drops such points)."""
    p = _cloud(points)
    n = p.size(1)
    if n == 0:
        return p.clone()
    v = np.float32(voxel_size)
    # torch's min / max propagate NaN, so one NaN coordinate makes its axis' bounds NaN
    origin, dims = _voxel_grid(p.min(dim=1)[0].cpu().numpy(), p.max(dim=1)[0].cpu().numpy(), v)
    out = torch.empty((3, n), dtype=torch.float32, device=p.device)
    count = torch.zeros(1, dtype=torch.int32, device=p.device)
    nbytes = _cabi.lib().s4g_voxel_down_sample_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    o3 = (ctypes.c_float * 3)(*[float(x) for x in origin])
    d3 = (ctypes.c_int32 * 3)(*[int(x) for x in dims])
    with torch.cuda.device(p.device):
        rc = _cabi.lib().s4g_voxel_down_sample_f32(p.data_ptr(), n, float(v), o3, d3, out.data_ptr(),
                                                   count.data_ptr(), ws.data_ptr(), nbytes,
                                                   _F._stream())
    _cabi.check(rc, "voxel_down_sample")
    return out[:, :int(count.item())].contiguous()


def radius_outlier_mask(points, nb_points=NUM_POINTS_THRESHOLD, radius=RADIUS_THRESHOLD):
    """Boolean keep mask of open3d's RemoveRadiusOutliers (more than nb_points points,
    the point itself included, within the radius)."""
    p = _cloud(points)
    n = p.size(1)
    keep = torch.zeros(n, dtype=torch.uint8, device=p.device)
    if n == 0:
        return keep.bool()
    nbytes = _cabi.lib().s4g_radius_outlier_workspace_bytes(n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=p.device)
    with torch.cuda.device(p.device):
        rc = _cabi.lib().s4g_radius_outlier_mask_f32(p.data_ptr(), n, float(radius), int(nb_points),
                                                     keep.data_ptr(), ws.data_ptr(), nbytes,
                                                     _F._DIST_FLAGS, _F._stream())
    _cabi.check(rc, "radius_outlier_mask")
    return keep.bool()


@dataclass(frozen=True)
class ViewProcessingConfig:
    """The constants of the data generator's `processing_and_trace` (data_gen/configs/config.py: WORKSPACE, VOXEL_SIZE,
    NUM_POINTS_THRESHOLD, RADIUS_THRESHOLD; the voxel bounds are the literals of the call,
    data_gen/pcd_classes/torch_precomputed_single_view_point_cloud.py:88-89).  They differ from the inference constants
    above."""
    workspace: tuple = (-0.40, 0.40, -0.35, 0.35, 0.749, 1.2)
    voxel_size: float = 0.005
    voxel_bounds: tuple = ((-0.5, -0.5, 0.7), (0.5, 0.5, 1.5))
    nb_points: int = 8
    radius: float = 0.04

    def grid(self):
        """(origin (3,) f32, dims (3,) int64) of the voxel grid; ValueError where it does not contain the crop box (the
        cell of a box face, in the kernel's fp32 arithmetic, outside [0, dims - 1])."""
        if not float(self.voxel_size) > 0.0:
            raise ValueError("voxel_size must be positive, got %r" % (self.voxel_size,))
        v = np.float32(self.voxel_size)
        try:
            origin, dims = _voxel_grid(self.voxel_bounds[0], self.voxel_bounds[1], v)
        except RuntimeError as e:
            raise ValueError(str(e))
        box = np.asarray(self.workspace, dtype=np.float32)
        for a in range(3):
            lo, hi = box[2 * a], box[2 * a + 1]
            if not lo < hi:                       # an empty (or NaN) box keeps nothing and asks nothing of the grid
                continue
            clo = np.floor(np.float32(np.float32(lo - origin[a]) / v))
            chi = np.floor(np.float32(np.float32(hi - origin[a]) / v))
            if not (clo >= 0 and chi <= dims[a] - 1):
                raise ValueError("voxel_bounds %r do not contain the workspace %r on axis %d"
                                 % (self.voxel_bounds, self.workspace, a))
        return origin, dims


@dataclass
class ProcessedViews:
    """What `process_views` returns: device tensors.  `points` (B, 3, N) fp32 the kept voxel means in ascending
    (iz, iy, ix) cell order, NaN from column count[b] on; `index_in_ref` (B, N) int32 per kept mean the highest original
    index among its voxel's points, -1 in the padding; `crop_count`, `voxel_count`, `count` (B,) int32 the rows after the
    crop, the voxels and the kept means."""
    points: torch.Tensor
    index_in_ref: torch.Tensor
    crop_count: torch.Tensor
    voxel_count: torch.Tensor
    count: torch.Tensor
    unbatched: bool = False

    def trace(self, reference):
        """reference (B, 3, N) (or (3, N) for one view), the noise-free points of the same pixels -> (B, 3, N):
        reference[b][:, index_in_ref[b]], NaN in the padding -- `reference_cloud` of the view-stage label calls."""
        ref = _F._f32c(reference, "reference")
        if ref.dim() == 2:
            ref = ref[None]
        if ref.shape != self.points.shape:
            raise RuntimeError("reference must be %s, got %s" % (tuple(self.points.shape), tuple(ref.shape)))
        if ref.device != self.points.device:
            raise RuntimeError("reference must live on the views' device")
        idx = self.index_in_ref.long()
        live = (idx >= 0)[:, None, :]
        got = torch.gather(ref, 2, idx.clamp_(min=0)[:, None, :].expand(-1, 3, -1))
        return torch.where(live, got, torch.full_like(got, float("nan")))


def process_views(clouds, count=None, config=None):
    """The data generator's `processing_and_trace` (data_gen/pcd_classes/torch_precomputed_single_view_point_cloud.py:
    64-97; the same code in torch_contact_single_view_point_cloud.py:79-112 and torch_precomputed_baseline.py:76-109)
    for B rendered views in one sync-free, graph-capturable call -> `ProcessedViews`.

    clouds (B, 3, N) fp32 (one view may be passed as (3, N) and gets a leading 1); count (B,) int32 on the device
    (optional): the rows of view b at or past count[b] (clamped to [0, N]) do not exist; config a
    `ViewProcessingConfig` (default: the data generator's constants).  Per view: the crop (`filter_work_space`), the
    voxel means over the grid of config.voxel_bounds (`voxel_down_sample`'s cells and means, cells ascending), the
    radius-outlier filter on those means (`radius_outlier_mask`, the distance mode of `functions.set_distance_mode`) --
    bit for bit what the three single-cloud functions give one after the other -- and `index_in_ref`, the reference's
    `arange(n)[valid][max(trace, axis=1)][valid3]`.  The voxel bounds must contain the workspace (ValueError): that
    is what makes the grid, the sort width and the launch chain independent of the data."""
    if not isinstance(clouds, torch.Tensor) or clouds.device.type != "cuda":
        raise RuntimeError("clouds must be a CUDA tensor (there is no CPU fallback)")
    if count is not None and (not isinstance(count, torch.Tensor) or count.device.type != "cuda"):
        raise RuntimeError("count must be a CUDA tensor (there is no CPU fallback)")
    cfg = ViewProcessingConfig() if config is None else config
    unbatched = clouds.dim() == 2
    if unbatched:
        clouds = clouds[None]
    xyz = _F._f32c(clouds, "clouds")
    if xyz.dim() != 3 or xyz.size(1) != 3:
        raise RuntimeError("clouds must be (B, 3, N)")
    B, _, N = xyz.shape
    if B > 65535 or B * N >= 2 ** 31:
        raise ValueError("process_views serves B <= 65535 views and B * N < 2^31 rows, got B = %d, N = %d" % (B, N))
    if not (0.0 < float(cfg.radius) < 1e18) or int(cfg.nb_points) < 0:
        raise ValueError("radius must be in (0, 1e18) and nb_points >= 0")
    origin, dims = cfg.grid()
    live = None
    if count is not None:
        if count.dtype != torch.int32:
            raise RuntimeError("count must be int32, got %s" % count.dtype)
        if tuple(count.shape) != (B,):
            raise RuntimeError("count must be (B,)")
        if count.device != xyz.device:
            raise RuntimeError("clouds and count must live on one device")
        live = count.contiguous()
    dev = xyz.device
    points = torch.empty((B, 3, N), dtype=torch.float32, device=dev)
    index = torch.empty((B, N), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 3), dtype=torch.int32, device=dev)
    nbytes = _cabi.lib().s4g_process_views_workspace_bytes(B, N)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    box = (ctypes.c_float * 6)(*[float(v) for v in cfg.workspace])
    o3 = (ctypes.c_float * 3)(*[float(x) for x in origin])
    d3 = (ctypes.c_int32 * 3)(*[int(x) for x in dims])
    with torch.cuda.device(dev):
        rc = _cabi.lib().s4g_process_views_f32(xyz.data_ptr(), None if live is None else live.data_ptr(), B, N, box,
                                               float(np.float32(cfg.voxel_size)), o3, d3, float(cfg.radius),
                                               int(cfg.nb_points), points.data_ptr(), index.data_ptr(),
                                               counts.data_ptr(), ws.data_ptr(), nbytes, _F._DIST_FLAGS, _F._stream())
    _cabi.check(rc, "process_views")
    per = counts.t().contiguous()
    return ProcessedViews(points, index, per[0], per[1], per[2], unbatched)


def _splitmix64(x):
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
        z = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)).astype(np.uint64)
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)).astype(np.uint64)
        return z ^ (z >> np.uint64(31))


def sample_indices(n, num_input, seed=0):
    """Seeded counterpart of `np.random.choice(n, num_input, replace=n < num_input)`
    (grasp_detector.py:86-89): a keyed permutation, repeated when the cloud is short."""
    if n <= 0:
        raise RuntimeError("cannot sample from an empty cloud")
    with np.errstate(over="ignore"):
        base = np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        keys = _splitmix64(np.arange(n, dtype=np.uint64) + base)
    perm = np.argsort(keys, kind="stable")
    if n >= num_input:
        return perm[:num_input]
    return np.tile(perm, (num_input + n - 1) // n)[:num_input]


class CloudPreProcessor:
    """Device counterpart of the reference class of the same name; `points` is (3, N)."""

    def __init__(self, cloud):
        self.points = _cloud(cloud)

    def filter_work_space(self, workspace=WORKSPACE):
        valid_index = filter_work_space(self.points, workspace)
        self.points = self.points[:, valid_index].contiguous()
        return valid_index

    def voxelize(self, voxel_size=VOXEL_SIZE):
        self.points = voxel_down_sample(self.points, voxel_size)

    def remove_outliers(self, nb_points=NUM_POINTS_THRESHOLD, radius=RADIUS_THRESHOLD):
        self.points = self.points[:, radius_outlier_mask(self.points, nb_points, radius)].contiguous()

    def estimate_normals(self, camera_pos=None):
        """`CloudPreProcessor.estimate_normals(camera_pos=np.zeros(3))` (cloud_processor.py:44-52): the normals of
        `points` by `postprocess.estimate_normals` with the reference's radius and max_nn, turned towards camera_pos
        (default: the origin), stored in `normals` (3, N)."""
        from .postprocess import estimate_normals as _estimate
        if camera_pos is None:
            cam = torch.zeros(3, dtype=torch.float32, device=self.points.device)
        else:
            cam = torch.as_tensor(camera_pos, dtype=torch.float32).reshape(3).to(self.points.device)
        self.normals = _estimate(self.points, cam).normals[0]
        return self.normals


def sample_single_cloud(points, num_input=25600, seed=0, mode="random"):
    """(3, N) -> (3, num_input).  mode "random": seeded permutation / repetition;
    "fps": farthest point sampling when N > num_input (the strategy the reference's
    comment at grasp_detector.py:84 proposes), same kernel as the network's sampler."""
    p = _cloud(points)
    n = p.size(1)
    if mode == "fps" and n > num_input:
        idx = _F.farthest_point_sample(p.unsqueeze(0), num_input)[0]
    elif mode in ("random", "fps"):
        idx = torch.from_numpy(sample_indices(n, num_input, seed).astype(np.int64)).to(p.device)
    else:
        raise ValueError("mode must be 'random' or 'fps'")
    return p[:, idx].contiguous()


def pre_processing(cloud, num_input=25600, seed=0, mode="random", workspace=None):
    """`GraspDetector._pre_processing`: (optional crop), voxelize, remove outliers,
    REAL2TRAIN transform, subsample.  Returns (points (3, num_input), processed cloud (3, M))."""
    cp = CloudPreProcessor(cloud)
    if workspace is not None:
        cp.filter_work_space(workspace)
    cp.voxelize()
    cp.remove_outliers()
    t = torch.tensor(REAL2TRAIN, dtype=torch.float32, device=cp.points.device)
    pts = (t[:3, :3] @ cp.points + t[:3, 3:4]).contiguous()
    return sample_single_cloud(pts, num_input, seed, mode), cp.points
