"""The rendered views the view stage starts from: data_gen/render/cycles_render.py of the reference without Blender.
Per scene and camera it writes a noise-free cloud (`process_views(...).trace(reference)`'s `reference`) and a noisy one
(`process_views`' `clouds`); here both come from posed triangle meshes in one sync-free call.  Host code only; the
kernels are csrc/render_views.hip (contract: include/s4g_ops.h, s4g_render_views_f32).  `postprocess` re-exports every
public name of this module, and this module reads `postprocess`'s host plumbing inside its calls.

What a maintainer should know (DESIGN.md has the reasons): the renderer is pinned by restatement only -- Cycles cannot
be run against it; K^-1 is written out, not inverted numerically; the range image is rounded to fp32 as Blender's pixel
buffer is; triangle edges are inclusive and the lowest triangle index wins a tie; the noise is a tensor of multipliers
the caller can see and fix; a miss reads +inf, not Cycles' far value (both fail the 5 m cut)."""
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _cabi
from . import functions as _F

__all__ = ["CAMERA_POSE", "MeshScene", "RenderConfig", "RenderedViews", "load_obj", "compose_mesh_scene",
           "batch_mesh_scenes", "render_views", "RENDER_MAX_VIEWS", "RENDER_MAX_PIXELS", "RENDER_MAX_TRIANGLES"]

# cycles_render.py:14-19: (x, y, z, qw, qx, qy, qz)
CAMERA_POSE = ((0.8, 0, 1.7, 0.948, 0, 0.317, 0),
               (-0.8, 0, 1.6, -0.94, 0, 0.342, 0),
               (0.0, 0.75, 1.7, 0.671, -0.224, 0.224, 0.671),
               (0.0, -0.75, 1.6, -0.658, -0.259, -0.259, 0.658))
RENDER_MAX_VIEWS = 65535                   # B * V: one grid row per view
RENDER_MAX_PIXELS = 1 << 22                # H * W
RENDER_MAX_TRIANGLES = 1 << 24             # exclusive


def load_obj(path):
    """A Wavefront OBJ file -> (vertices (n, 3) float32, faces (m, 3) int64).  Only `v` and `f` lines are read; a
    polygon is fanned from its first vertex; `a/b/c` forms keep the vertex index; negative indices count from the last
    vertex read so far."""
    verts, faces = [], []
    with open(path, "r") as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(tok[1]), float(tok[2]), float(tok[3])])
            elif tok[0] == "f":
                idx = []
                for w in tok[1:]:
                    i = int(w.split("/")[0])
                    if i == 0:
                        raise ValueError("%s: OBJ indices start at 1" % path)
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                if len(idx) < 3:
                    raise ValueError("%s: a face needs three vertices" % path)
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("%s: a face names a vertex the file does not have" % path)
    return v, f


@dataclass
class MeshScene:
    """One scene as a triangle soup: `triangles` (T, 3, 3) fp32 in the world frame, `labels` (T,) int32 the object
    label of every triangle."""
    triangles: torch.Tensor
    labels: torch.Tensor


def compose_mesh_scene(meshes, poses, labels=None, device="cuda"):
    """meshes: a list of (vertices (n, 3), faces (m, 3)) as `load_obj` returns them; poses: one (x, y, z, qw, qx, qy,
    qz) each; labels: one int each (default 0, 1, ...) -> `MeshScene` on `device`.  Every mesh is moved by
    `pose_matrix(pose)` in float64 and rounded to fp32 once, as the scene generator places its objects."""
    from .postprocess import pose_matrix
    if len(meshes) != len(poses):
        raise ValueError("one pose per mesh: %d meshes, %d poses" % (len(meshes), len(poses)))
    if labels is None:
        labels = list(range(len(meshes)))
    if len(labels) != len(meshes):
        raise ValueError("one label per mesh")
    tris, labs = [], []
    for (v, f), pose, lab in zip(meshes, poses, labels):
        v = torch.as_tensor(np.asarray(v), dtype=torch.float64).reshape(-1, 3)
        f = torch.as_tensor(np.asarray(f), dtype=torch.int64).reshape(-1, 3)
        if f.numel() and (int(f.min()) < 0 or int(f.max()) >= v.size(0)):
            raise ValueError("a face names a vertex the mesh does not have")
        m = pose_matrix(pose)
        w = (v @ m[:3, :3].t() + m[:3, 3]).float()
        tris.append(w[f])
        labs.append(torch.full((f.size(0),), int(lab), dtype=torch.int32))
    if tris:
        t, l = torch.cat(tris), torch.cat(labs)
    else:
        t, l = torch.zeros((0, 3, 3), dtype=torch.float32), torch.zeros((0,), dtype=torch.int32)
    return MeshScene(t.to(device).contiguous(), l.to(device).contiguous())


def batch_mesh_scenes(scenes):
    """A list of `MeshScene` -> (triangles (B, T, 3, 3) fp32, labels (B, T) int32, tri_count (B,) int32) on the first
    scene's device, T the longest scene; the rows past a scene's count hold NaN and label -1."""
    if not scenes:
        raise ValueError("no scenes")
    dev = scenes[0].triangles.device
    T = max(int(s.triangles.size(0)) for s in scenes)
    tri = torch.full((len(scenes), T, 3, 3), float("nan"), dtype=torch.float32, device=dev)
    lab = torch.full((len(scenes), T), -1, dtype=torch.int32, device=dev)
    for b, s in enumerate(scenes):
        n = int(s.triangles.size(0))
        tri[b, :n] = s.triangles.to(dev)
        lab[b, :n] = s.labels.to(dev)
    cnt = torch.tensor([int(s.triangles.size(0)) for s in scenes], dtype=torch.int32).to(dev)
    return tri, lab, cnt


@dataclass(frozen=True)
class RenderConfig:
    """The constants of cycles_render.py: the image and K of :25-28, the cut of :134, CAMERA_POSE of :14-19 and the
    noise of BlensorSceneServer (:126; BlensorSceneDuplicate uses 0.003, :222)."""
    width: int = 640
    height: int = 480
    fx: float = 700.0
    fy: float = 700.0
    cx: float = 320.0
    cy: float = 240.0
    max_depth: float = 5.0
    camera_poses: tuple = CAMERA_POSE
    noise_sigma: float = 0.005

    def check(self):
        if int(self.width) <= 0 or int(self.height) <= 0 or int(self.width) * int(self.height) > RENDER_MAX_PIXELS:
            raise ValueError("the image needs 0 < width * height <= 2^22, got %r x %r" % (self.width, self.height))
        for name in ("fx", "fy"):
            v = float(getattr(self, name))
            if not (0.0 < v < float("inf")):
                raise ValueError("%s must be positive and finite, got %r" % (name, v))
        for name in ("cx", "cy"):
            if not np.isfinite(float(getattr(self, name))):
                raise ValueError("%s must be finite" % name)
        if len(self.camera_poses) < 1:
            raise ValueError("no cameras")

    def cameras(self):
        """(V, 12) float64: per camera its camera-to-world rotation (`quaternion_matrix`, row-major) and its centre."""
        from .postprocess import quaternion_matrix
        rows = []
        for pose in self.camera_poses:
            p = [float(v) for v in pose]
            if len(p) != 7:
                raise ValueError("a camera pose is (x, y, z, qw, qx, qy, qz)")
            rows.append(torch.cat([quaternion_matrix(p[3:]).reshape(9), torch.tensor(p[:3], dtype=torch.float64)]))
        return torch.stack(rows)


@dataclass
class RenderedViews:
    """What `render_views` returns: device tensors, P = H * W.  Dense: `range` (B, V, P) fp32 ray lengths, +inf on a
    miss; `triangle` (B, V, P) int32, -1 on a miss; `label` (B, V, P) int32 the hit triangle's scene label, -1 on a
    miss (None without labels).  Compact, the kept pixels in ascending pixel index: `points` and `noisy` (B, V, 3, P)
    fp32 (NaN from count on; `noisy` is None with noise=False), `pixel` (B, V, P) int32 (-1 from count on), `count`
    (B, V) int32."""
    range: torch.Tensor
    triangle: torch.Tensor
    points: torch.Tensor
    noisy: torch.Tensor
    pixel: torch.Tensor
    count: torch.Tensor
    label: torch.Tensor
    config: RenderConfig = field(default_factory=RenderConfig)

    def clouds(self, noisy=True):
        """((B * V, 3, P) fp32, (B * V,) int32): `process_views`' clouds and count (noisy=True), or the `reference`
        of its `.trace` (noisy=False)."""
        src = self.noisy if noisy else self.points
        if src is None:
            raise RuntimeError("these views were rendered without a noisy cloud")
        B, V, _, P = src.shape
        return src.reshape(B * V, 3, P), self.count.reshape(B * V)

    def dump(self, b, v):
        """(cloud (n, 3), noisy cloud (n, 3) or None) as numpy: the two files the reference writes for scene b and
        camera v (a host read)."""
        n = int(self.count[b, v].item())
        pts = self.points[b, v, :, :n].t().contiguous().cpu().numpy()
        nsy = None if self.noisy is None else self.noisy[b, v, :, :n].t().contiguous().cpu().numpy()
        return pts, nsy


def _cuda(t, name):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError("%s must be a CUDA tensor (there is no CPU fallback)" % name)


def render_views(scene, tri_count=None, config=None, noise=None, generator=None, labels=None):
    """Range images and clouds of B scenes from the V cameras of `config` in one sync-free, graph-capturable call ->
    `RenderedViews`.

    scene: a `MeshScene`, a list of them (padded by `batch_mesh_scenes`), or a CUDA tensor of triangles (T, 3, 3) /
    (B, T, 3, 3) fp32 with `tri_count` (B,) int32 on the device (optional: the rows of scene b at or past tri_count[b],
    clamped to [0, T], do not exist) and `labels` (B, T) int32 (optional).  noise: None draws 1 + noise_sigma * randn
    (float64, `generator`) on the device; False renders no noisy cloud; a (B, V, H * W) float64 CUDA tensor gives the
    multipliers themselves.  Limits (ValueError): B * V <= 65 535, H * W <= 2^22, T < 2^24."""
    from .postprocess import _small_on_device, _workspace
    cfg = RenderConfig() if config is None else config
    cfg.check()
    if isinstance(scene, MeshScene):
        tri, lab = scene.triangles[None], scene.labels[None]
    elif isinstance(scene, (list, tuple)):
        if tri_count is not None:
            raise ValueError("a list of scenes carries its own counts")
        tri, lab, tri_count = batch_mesh_scenes(list(scene))
    else:
        tri, lab = scene, labels
        _cuda(tri, "scene")
        if tri.dim() == 3:
            tri = tri[None]
            lab = None if lab is None else lab[None] if lab.dim() == 1 else lab
    _cuda(tri, "scene")
    if tri.dtype != torch.float32:
        raise RuntimeError("triangles must be float32, got %s" % tri.dtype)
    if tri.dim() != 4 or tuple(tri.shape[2:]) != (3, 3):
        raise RuntimeError("triangles must be (B, T, 3, 3)")
    tri = tri.contiguous()
    dev = tri.device
    B, T = int(tri.size(0)), int(tri.size(1))
    cam = cfg.cameras()
    V, H, W = int(cam.size(0)), int(cfg.height), int(cfg.width)
    P = H * W
    if B * V > RENDER_MAX_VIEWS or T >= RENDER_MAX_TRIANGLES:
        raise ValueError("render_views serves B * V <= 65535 views and T < 2^24 triangles, got B = %d, V = %d, T = %d"
                         % (B, V, T))
    cnt = None
    if tri_count is not None:
        _cuda(tri_count, "tri_count")
        if tri_count.dtype != torch.int32:
            raise RuntimeError("tri_count must be int32, got %s" % tri_count.dtype)
        if tuple(tri_count.shape) != (B,):
            raise RuntimeError("tri_count must be (B,)")
        if tri_count.device != dev:
            raise RuntimeError("triangles and tri_count must live on one device")
        cnt = tri_count.contiguous()
    if lab is not None:
        _cuda(lab, "labels")
        if lab.dtype != torch.int32 or tuple(lab.shape) != (B, T) or lab.device != dev:
            raise RuntimeError("labels must be (B, T) int32 on the triangles' device")
    mult = None
    if noise is None:
        mult = 1.0 + float(cfg.noise_sigma) * torch.randn((B, V, P), dtype=torch.float64, device=dev,
                                                          generator=generator)
    elif noise is not False:
        _cuda(noise, "noise")
        if noise.dtype != torch.float64 or tuple(noise.shape) != (B, V, P) or noise.device != dev:
            raise RuntimeError("noise must be (B, V, H * W) float64 on the triangles' device")
        mult = noise.contiguous()
    # by value through the bounded cache: the first call with these cameras copies, the next ones do not
    cams = _small_on_device(cam, torch.float64, dev)[None].expand(B, V, 12).contiguous()
    rng = torch.empty((B, V, P), dtype=torch.float32, device=dev)
    idx = torch.empty((B, V, P), dtype=torch.int32, device=dev)
    pts = torch.empty((B, V, 3, P), dtype=torch.float32, device=dev)
    nsy = None if mult is None else torch.empty((B, V, 3, P), dtype=torch.float32, device=dev)
    pix = torch.empty((B, V, P), dtype=torch.int32, device=dev)
    count = torch.empty((B, V), dtype=torch.int32, device=dev)
    L = _cabi.lib()
    ws, nbytes = _workspace(L.s4g_render_views_workspace_bytes(B, V, T, H, W), dev)
    with torch.cuda.device(dev):
        rc = L.s4g_render_views_f32(tri.data_ptr() if T else None, None if cnt is None else cnt.data_ptr(),
                                    cams.data_ptr(), B, V, T, float(cfg.fx), float(cfg.fy), float(cfg.cx),
                                    float(cfg.cy), float(cfg.max_depth), H, W,
                                    None if mult is None else mult.data_ptr(), rng.data_ptr(), idx.data_ptr(),
                                    pts.data_ptr(), None if nsy is None else nsy.data_ptr(), pix.data_ptr(),
                                    count.data_ptr(), ws.data_ptr(), nbytes, _F._stream())
    _cabi.check(rc, "render_views")
    label = None
    if lab is not None:
        if T == 0:
            label = torch.full((B, V, P), -1, dtype=torch.int32, device=dev)
        else:
            got = torch.gather(lab[:, None, :].expand(B, V, T), 2, idx.clamp(min=0).long())
            label = torch.where(idx >= 0, got, torch.full_like(got, -1))
    return RenderedViews(rng, idx, pts, nsy, pix, count, label, cfg)
