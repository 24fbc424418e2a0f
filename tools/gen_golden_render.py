#!/usr/bin/env python3
"""Writes tests/golden/render_views.npz: the fixture of `render_views`.

    python tools/gen_golden_render.py --mesh <the reference tree>/objects/mesh/camera.obj

It holds the mesh (fp32 vertices, uint16 faces), the offset that stands it on the table box of
tests/render_ref.py (top at z = 0.75), the reference's four camera poses, a fifth pose (camera 0 moved along its
viewing direction to 0.35 m from the object, so that the mesh fills the image), and per view the yardstick's dense
range and triangle maps at 160 x 120 with the intrinsics scaled by 0.25, plus its `decided` mask.  The yardstick
scans every triangle per pixel (about a minute and a half per view); the views run in parallel processes.  At most
1 % of a view's pixels may be undecided."""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import render_ref as RR  # noqa: E402

SCALE = 0.25
CLOSE = 0.35


def load_obj(path):
    sys.path.insert(0, ROOT)
    from s4g_release_amd.render import load_obj as _load
    return _load(path)


def _view(args):
    tri, R, c = args
    res = RR.render_ref(tri, R, c, RR.intrinsics(SCALE))
    return res.range, res.triangle, res.decided


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "render_views.npz"))
    a = ap.parse_args()
    vertices, faces = load_obj(a.mesh)
    vertices = np.asarray(vertices, np.float32)
    faces = np.asarray(faces, np.int64)
    assert faces.max() < 65536
    lo, hi = vertices.astype(np.float64).min(axis=0), vertices.astype(np.float64).max(axis=0)
    offset = np.array([-(lo[0] + hi[0]) / 2, -(lo[1] + hi[1]) / 2, RR.TABLE_HI[2] - lo[2]], dtype=np.float64)
    poses = np.asarray(RR.CAMERA_POSE, np.float64)
    R0, c0 = RR.camera(poses[0])
    centre = (lo + hi) / 2 + offset
    forward = R0 @ np.array([0.0, 0.0, -1.0])
    close = poses[0].copy()
    close[:3] = c0 + (np.dot(centre - c0, forward) - CLOSE) * forward
    g = {"vertices": vertices, "faces": faces.astype(np.uint16), "mesh_offset": offset, "poses": poses,
         "close_pose": close, "scale": np.float64(SCALE)}
    tri = RR.fixture_scene(g)
    views = RR.fixture_views(g)
    with Pool(len(views)) as pool:
        maps = pool.map(_view, [(tri, R, c) for _, R, c in views])
    K = RR.intrinsics(SCALE)
    for (name, _, _), (rng, idx, decided) in zip(views, maps):
        und = int((~decided).sum())
        print("%s: %d of %d pixels hit, %d on the mesh, %d undecided" % (
            name, int((idx >= 0).sum()), K.H * K.W, int(((idx >= 0) & (idx < len(faces))).sum()), und))
        assert und <= 0.01 * K.H * K.W, name
        g[name + "/range"] = rng
        g[name + "/triangle"] = idx.astype(np.int32)
        g[name + "/decided"] = np.packbits(decided)
    np.savez_compressed(a.out, **g)
    print("wrote %s: %d bytes" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
