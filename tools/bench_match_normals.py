#!/usr/bin/env python3
"""Times the normal matching (`postprocess.match_normals`) and the labelling call that starts with it
(`postprocess.label_view(match_normal=True)`), in one process, per scene size of `--scene-points`:

  (a) match_normals                       the whole call: grid build + query kernel
  (b) the grid build                      the same call with ONE view point per scene (the query kernel has nothing to do)
  (c) the library's own index-order scan  the same inputs plus one scene point 1e4 m away, which takes the scene out of
                                          the grid's exactness range: every query scans every scene point
  (d) label_view(match_normal=True)       on `--label-scenes` of the scenes: match_normals + index selection +
                                          estimate_frames + grade_local_search; (a)'s share is taken on the same scenes
  (e) the reference-shaped formulation    the per-point loop of torch_single_view_point_cloud.py:137-141 restated on the
                                          device (a distance row, the radius mask, `topk` where the cap cuts, a mean), run
                                          on `--loop-points` view points of one scene and scaled to B * N

Shape: `--scenes` views of `--points` points against scenes of M points: cylinders of 3 cm radius on a 0.1 m pitch over
a 0.6 m table top, sampled at the fixture's density (tests/golden/match_normals.npz: about 90 points per 1 cm ball), as
many of them as M holds, the rest of M on the table; the view is scene points above the sample region jittered by
2 mm.  Method: warm-up, then `--repeat` rounds of `--inner` calls between device events; the median and the spread per
leg.  One JSON line per scene size."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PER_OBJECT = 5300


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def make_scene(rng, M, N, th):
    from tools.gen_golden_darboux import cylinder_points
    n_obj = max(1, int(0.95 * M) // PER_OBJECT)
    parts = [cylinder_points(rng, (0.05 + 0.1 * (o % 6), 0.05 + 0.1 * (o // 6)), 0.03, 0.10, PER_OBJECT, 1 + o, th)
             for o in range(n_obj)]
    nt = M - n_obj * PER_OBJECT
    parts.append((np.stack([rng.uniform(0, 0.6, nt), rng.uniform(0, 0.6, nt), np.full(nt, th)], 1),
                  np.tile([0, 0, 1.0], (nt, 1)), np.zeros(nt, int)))
    pts, nrm, lab = (np.concatenate([p[i] for p in parts]) for i in range(3))
    nrm = nrm + rng.normal(0, 0.05, nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o = rng.permutation(M)
    pts, nrm, lab = pts[o], nrm[o], lab[o]
    up = np.nonzero(pts[:, 2] > th + 0.025)[0]
    view = pts[rng.choice(up, N, replace=len(up) < N)] + rng.normal(0, 0.002, (N, 3))
    return pts.T.astype(np.float32), nrm.T.astype(np.float32), lab.astype(np.int32), view.T.astype(np.float32)


def reference_loop(view, pts, nrm, radius, max_nn):
    """:137-141 per view point, as written, with the hybrid search as a distance row."""
    out = []
    for i in range(view.shape[0]):
        d2 = ((pts - view[i]) ** 2).sum(1)
        idx = torch.nonzero(d2 < radius * radius)[:, 0]
        if idx.shape[0] > max_nn:
            idx = idx[torch.topk(d2[idx], max_nn, largest=False).indices]
        out.append(nrm[idx].mean(0))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--points", type=int, default=25600)
    ap.add_argument("--scene-points", type=int, nargs="+", default=[200000, 65536])
    ap.add_argument("--label-scenes", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--loop-points", type=int, default=48)
    args = ap.parse_args()
    from s4g_release_amd import postprocess as PP
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    radius, max_nn = PP.CURVATURE_RADIUS, PP.NORMAL_MAX_NN
    th = PP.LocalSearchConfig().table_height
    B, N = args.scenes, args.points
    for M in args.scene_points:
        rng = np.random.default_rng(M)
        scenes = [make_scene(rng, M, N, th) for _ in range(B)]
        pts, nrm, lab, view = (torch.from_numpy(np.stack([s[i] for s in scenes])).to(dev) for i in range(4))
        cam = torch.tensor([0.9, -0.3, th + 0.8], device=dev)
        far = torch.full((B, 3, 1), 1e4, device=dev)
        pts_far, nrm_far = torch.cat([pts, far], 2).contiguous(), torch.cat([nrm, far * 0 + 1], 2).contiguous()
        Bl = min(args.label_scenes, B)
        leg_a = lambda: PP.match_normals(view, pts, nrm, cam, radius, max_nn)
        leg_b = lambda: PP.match_normals(view[:, :, :1], pts, nrm, cam, radius, max_nn)
        leg_c = lambda: PP.match_normals(view, pts_far, nrm_far, cam, radius, max_nn)
        leg_a2 = lambda: PP.match_normals(view[:Bl], pts[:Bl], nrm[:Bl], cam, radius, max_nn)
        leg_d = lambda: PP.label_view(view[:Bl], None, pts[:Bl], nrm[:Bl], lab[:Bl], radius=radius, match_normal=True,
                                      camera=cam, max_nn=max_nn)
        m = leg_a()
        scan = leg_c()
        v = leg_d()
        torch.cuda.synchronize()
        # the scan finds the same sets and adds in the same order: the same bits
        same = bool(torch.equal(m.normals.view(torch.int32), scan.normals.view(torch.int32))
                    and torch.equal(m.count, scan.count) and torch.equal(m.flags, scan.flags))
        nl = min(args.loop_points, N)
        leg_e = lambda: reference_loop(view[0].t()[:nl].contiguous(), pts[0].t().contiguous(), nrm[0].t().contiguous(),
                                       radius, max_nn)
        loop = torch.nn.functional.normalize(leg_e(), dim=1)
        got = m.normals[0].t()[:nl]
        loop_err = float(torch.minimum((got - loop).abs().amax(1), (got + loop).abs().amax(1)).max())   # modulo the orientation
        te = float(np.median([timed(leg_e, 1) for _ in range(2)])) * B * N / nl
        legs = {"a": leg_a, "b": leg_b, "c": leg_c, "a2": leg_a2, "d": leg_d}
        inner = {"a": args.inner, "b": args.inner, "c": 1, "a2": args.inner, "d": 1}
        t = {k: [] for k in legs}
        for i in range(args.repeat):
            order = list(legs) if i % 2 == 0 else list(legs)[::-1]
            for k in order:
                if k in ("c", "d") and i >= 3:                 # the long legs: three rounds
                    continue
                t[k].append(timed(legs[k], inner[k]))
        med = {k: float(np.median(x)) for k, x in t.items()}
        spread = {k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()}
        k = m.count.float()
        print(json.dumps({
            "B": B, "N": N, "M": M, "radius": radius, "max_nn": max_nn,
            "match_normals_ms": round(med["a"], 3), "match_normals_min_max_ms": spread["a"],
            "grid_build_ms": round(med["b"], 3), "grid_build_min_max_ms": spread["b"],
            "query_kernel_ms": round(med["a"] - med["b"], 3),
            "index_scan_ms": round(med["c"], 3), "index_scan_min_max_ms": spread["c"],
            "scan_over_grid": round(med["c"] / med["a"], 1), "scan_gives_the_same_bits": same,
            "queries_per_second": round(B * N / (med["a"] * 1e-3)),
            "label_scenes": Bl, "label_view_ms": round(med["d"], 3), "label_view_min_max_ms": spread["d"],
            "match_normals_on_those_scenes_ms": round(med["a2"], 3),
            "matching_share_of_label_view": round(med["a2"] / med["d"], 4),
            "reference_loop_ms_scaled": round(te, 1), "reference_loop_points_run": nl,
            "speedup_over_the_loop": round(te / med["a"], 1), "largest_distance_from_the_loop": loop_err,
            "kept_median": float(k.median()), "capped": int(m.capped.sum()), "empty": int(m.empty.sum()),
            "valid_frames": int(v.search.count.sum())}), flush=True)
        del pts, nrm, lab, view, pts_far, nrm_far, m, scan, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
