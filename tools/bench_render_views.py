#!/usr/bin/env python3
"""Times `render_views` on the device and prints one JSON line per configuration (profiles/r31_render_views.md).

    python tools/bench_render_views.py [--reps 5] [--scenes 1 16] [--copies 1 10]

Per configuration: B scenes x 4 cameras x 640 x 480, the fixture's mesh on its table (about 30 000 triangles) or
`copies` posed copies of it (ten: about 300 000).  Reported:
  call_ms          device events around `reps` calls after a warm-up, noise multipliers given (no random draw timed);
  survivors        triangles whose screen box touches a 16 x 16 tile, mean and maximum over the tiles (the boxes are
                   recomputed here in torch float64 with the kernel's rule);
  tests_per_s      (survivors summed over tiles) x 256 pixel threads / call time: the ray-triangle tests the cast
                   kernel executes per second of the WHOLE call (set-up and compaction included);
  scan_ms          the reference-shaped scan -- every ray against every triangle, no culling -- in torch float64 on the
                   same device, chunked, timed on `--scan-pixels` pixels of one view and scaled to the call's pixels;
  parity           the scan's nearest triangle against the kernel's on those pixels.
Blender's own time cannot be measured here (it is not installed); the scan is the stand-in."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from s4g_release_amd import postprocess as PP  # noqa: E402
from tests import render_ref as RR  # noqa: E402

TILE = 16


def build_scene(golden, copies, dev):
    verts = golden["vertices"]
    faces = golden["faces"].astype(np.int64)
    off = golden["mesh_offset"]
    rng = np.random.default_rng(0)
    meshes, poses = [], []
    for k in range(copies):
        if k == 0:
            pose = (off[0], off[1], off[2], 1.0, 0.0, 0.0, 0.0)
        else:
            a = rng.uniform(0, 2 * np.pi)
            pose = (off[0] + rng.uniform(-0.28, 0.28), off[1] + rng.uniform(-0.25, 0.25), off[2],
                    np.cos(a / 2), 0.0, 0.0, np.sin(a / 2))
        meshes.append((verts, faces))
        poses.append(pose)
    box = RR.box_triangles(RR.TABLE_LO, RR.TABLE_HI)
    scene = PP.compose_mesh_scene(meshes, poses, device=dev)
    tri = torch.cat([scene.triangles, torch.from_numpy(box).to(dev)])
    return tri.contiguous()


def survivors(tri, cam, cfg):
    """Triangles per tile by the kernel's box rule, torch float64: (mean, max, sum) over the tiles of one view."""
    R, c = cam[:9].reshape(3, 3), cam[9:]
    v = (tri.double() - c) @ R                                         # R^T (p - c)
    z = -v[..., 2]
    behind = (z <= 0).sum(dim=1)
    x = cfg.cx + cfg.fx * (v[..., 0] / z)
    y = cfg.cy + cfg.fy * (v[..., 1] / z)
    W, H = cfg.width, cfg.height
    x0 = (x.min(dim=1)[0].floor() - 1).clamp(0, W)
    x1 = (x.max(dim=1)[0].floor() + 1).clamp(-1, W - 1)
    y0 = (y.min(dim=1)[0].floor() - 1).clamp(0, H)
    y1 = (y.max(dim=1)[0].floor() + 1).clamp(-1, H - 1)
    full = (behind > 0) & (behind < 3)
    x0, x1 = torch.where(full, torch.zeros_like(x0), x0), torch.where(full, torch.full_like(x1, W - 1), x1)
    y0, y1 = torch.where(full, torch.zeros_like(y0), y0), torch.where(full, torch.full_like(y1, H - 1), y1)
    live = (behind < 3) & (x0 <= x1) & (y0 <= y1)
    tx0, tx1 = (x0[live] // TILE).long(), (x1[live] // TILE).long()
    ty0, ty1 = (y0[live] // TILE).long(), (y1[live] // TILE).long()
    nx, ny = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    grid = torch.zeros((ny + 1, nx + 1), dtype=torch.int64, device=tri.device)
    one = torch.ones_like(tx0)
    for yy, xx, s in ((ty0, tx0, 1), (ty0, tx1 + 1, -1), (ty1 + 1, tx0, -1), (ty1 + 1, tx1 + 1, 1)):
        grid.view(-1).index_add_(0, yy * (nx + 1) + xx, s * one)
    per = grid.cumsum(0).cumsum(1)[:ny, :nx]
    return float(per.double().mean()), int(per.max()), int(per.sum())


def scan(tri, cam, cfg, pix, chunk):
    """Every ray of `pix` against every triangle, nearest hit (lowest index on ties): torch float64, chunked."""
    R, c = cam[:9].reshape(3, 3), cam[9:]
    v = (tri.double() - c) @ R
    v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    Q = -torch.linalg.cross(v0, e1)
    Tn = (e2 * Q).sum(dim=1)
    rx = ((pix % cfg.width).double() + 0.5 - cfg.cx) / cfg.fx
    ry = ((pix // cfg.width).double() + 0.5 - cfg.cy) / cfg.fy
    best = torch.full((len(pix),), -1, dtype=torch.int64, device=tri.device)
    for s in range(0, len(pix), chunk):
        x, y = rx[s:s + chunk, None], ry[s:s + chunk, None]
        px, py, pz = y * e2[:, 2] + e2[:, 1], -e2[:, 0] - x * e2[:, 2], x * e2[:, 1] - y * e2[:, 0]
        det = e1[:, 0] * px + e1[:, 1] * py + e1[:, 2] * pz
        U = -(v0[:, 0] * px + v0[:, 1] * py + v0[:, 2] * pz)
        V = x * Q[:, 0] + y * Q[:, 1] - Q[:, 2]
        hit = ((det > 0) & (U >= 0) & (V >= 0) & (U + V <= det) & (Tn > 0)) | \
              ((det < 0) & (U <= 0) & (V <= 0) & (U + V >= det) & (Tn < 0))
        t = torch.where(hit, Tn / det, torch.full_like(det, float("inf")))
        bt, bi = t.min(dim=1)
        # torch.min does not promise the first of equal minima: take the lowest index that reaches it
        ids = torch.arange(t.size(1), device=t.device)[None].expand_as(t)
        first = torch.where(t == bt[:, None], ids, torch.full_like(ids, t.size(1))).min(dim=1)[0]
        best[s:s + chunk] = torch.where(torch.isfinite(bt), first, torch.full_like(bi, -1))
    return best


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--copies", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--scan-pixels", type=int, default=4096)
    ap.add_argument("--scan-budget", type=int, default=1 << 25, help="ray x triangle pairs per scan chunk")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_views needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    with np.load(os.path.join(ROOT, "tests", "golden", "render_views.npz")) as z:
        golden = {k: z[k] for k in z.files}
    cfg = PP.RenderConfig()
    cams = cfg.cameras().to(dev)
    V, P = cams.size(0), cfg.width * cfg.height
    for copies in a.copies:
        tri = build_scene(golden, copies, dev)
        T = tri.size(0)
        surv = [survivors(tri, cams[v], cfg) for v in range(V)]
        pix = torch.from_numpy(np.sort(np.random.default_rng(1).choice(P, a.scan_pixels, replace=False))).to(dev)
        chunk = max(1, a.scan_budget // T)
        scan_ms = timed(lambda: scan(tri, cams[0], cfg, pix, chunk), 2)
        for B in a.scenes:
            batch = tri[None].expand(B, T, 3, 3).contiguous()
            noise = 1.0 + cfg.noise_sigma * torch.randn((B, V, P), dtype=torch.float64, device=dev)
            out = PP.render_views(batch, config=cfg, noise=noise)
            same = bool((scan(tri, cams[0], cfg, pix, chunk) == out.triangle[0, 0][pix].long()).all())
            again = PP.render_views(batch, config=cfg, noise=noise)
            identical = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in
                            ((out.range, again.range), (out.triangle, again.triangle), (out.points, again.points),
                             (out.noisy, again.noisy), (out.pixel, again.pixel), (out.count, again.count)))
            del again
            ms = timed(lambda: PP.render_views(batch, config=cfg, noise=noise), a.reps)
            tests = sum(s[2] for s in surv) * TILE * TILE * B
            print(json.dumps({
                "scenes": B, "views": V, "width": cfg.width, "height": cfg.height, "triangles": T,
                "call_ms": round(ms, 3), "ms_per_view": round(ms / (B * V), 4),
                "survivors_mean": round(float(np.mean([s[0] for s in surv])), 1),
                "survivors_max": max(s[1] for s in surv),
                "tests_per_s": float("%.4g" % (tests / (ms * 1e-3))),
                "kept_per_view": int(out.count.double().mean()),
                "scan_ms_scaled": round(scan_ms * (B * V * P) / a.scan_pixels, 1),
                "scan_over_call": round(scan_ms * (B * V * P) / a.scan_pixels / ms, 1),
                "parity_with_scan": same, "run_to_run_identical": identical}), flush=True)
            del batch, noise, out


if __name__ == "__main__":
    main()
