#!/usr/bin/env python3
"""Times the batched frame grading (`postprocess.eval_frames`) against its two yardsticks, in one process:

  (a) eval_frames                         the new call
  (b) view_non_collision                  the existing collision counter on the same inputs: the floor the two shared
                                          counts already cost
  (c) the reference-shaped formulation    the per-pose torch loop of eval_experiment/eval_point_cloud.py:64-113 restated
                                          here on the device (boolean-mask compactions, torch.unique, one .cpu() per
                                          pose), run on `--loop-poses` poses of one scene and scaled to the pose count

Shape: B = 16 scenes of 200 000 points (the fixture's tabletop scene, tests/golden/post_eval.npz, resampled with a
0.3 mm jitter), K = 50 poses per scene, and K = 2 048 rows of which a device-side count of 300 are poses.
Method: warm-up, then `--repeat` rounds in which the legs run in alternating order; the median per leg, device events
around `--inner` calls.  Prints one JSON line per K."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reference_loop(g2l, xyz_homo, normals, labels, g):
    """eval_point_cloud.py:64-113 per pose, as written (one host read per pose)."""
    out = []
    nd = torch.tensor(g.neighbor_depth, device=xyz_homo.device)
    for T in g2l:
        res = {"antipodal_score": 0, "collision": False, "multi_objects": False}
        local = torch.matmul(T, xyz_homo)
        ln = torch.matmul(T[0:3, 0:3], normals)
        cp = (local[0] < g.finger_length) & (local[0] > -g.bottom_length)
        p = local[:, cp][0:3]
        zin = (p[2] < g.half_hand_thickness) & (p[2] > -g.half_hand_thickness)
        back = (p[1] < g.half_bottom_width) & (p[1] > -g.half_bottom_width) & (p[0] < -g.back_collision_margin) & zin
        if torch.sum(back) > g.back_collision_threshold:
            res["collision"] = True
        fl = (p[1] < g.half_bottom_width) & (p[1] > g.half_bottom_space)
        fr = (p[1] > -g.half_bottom_width) & (p[1] < -g.half_bottom_space)
        if torch.sum(zin & (fl | fr)) > g.finger_collision_threshold:
            res["collision"] = True
        cr = zin & (p[1] < g.half_bottom_space) & (p[1] > -g.half_bottom_space)
        if torch.unique(labels[cp][cr], sorted=False).shape[0] > 1:
            res["multi_objects"] = True
        cn = ln[:, cp][:, cr]
        cc = p[:, cr]
        if cc.shape[1] >= g.close_region_min_points and not (res["collision"] or res["multi_objects"]):
            ly, ry = torch.max(cc[1]), torch.min(cc[1])
            d = torch.min((ly - ry) / 3, nd)
            lm = torch.abs(cn[1, cc[1] > ly - d]).mean()
            rm = torch.abs(cn[1, cc[1] < ry + d]).mean()
            res["antipodal_score"] = (lm * rm).cpu().numpy()
        out.append(res)
    return out


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--loop-poses", type=int, default=48)
    args = ap.parse_args()
    from s4g_release_amd import postprocess as PP
    from tests import golden_util as GU
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    fx = GU.load("post_eval.npz")
    rng = np.random.default_rng(0)
    B, N = args.scenes, args.points
    idx = rng.integers(0, fx["cloud"].shape[1], (B, N))
    cloud = np.stack([fx["cloud"][:, i] for i in idx]) + rng.normal(0, 3e-4, (B, 3, N)).astype(np.float32)
    xyz = torch.from_numpy(cloud.astype(np.float32)).to(dev)
    nrm = torch.from_numpy(np.stack([fx["normals"][:, i] for i in idx])).to(dev)
    lab = torch.from_numpy(np.stack([fx["labels"][i] for i in idx])).to(dev)
    g = PP.GripperConfig()
    for K, live in ((50, None), (2048, 300)):
        poses = fx["poses"][rng.integers(0, len(fx["poses"]), (B, K))].copy()
        poses[..., :3, 3] += rng.uniform(-0.002, 0.002, (B, K, 3)).astype(np.float32)
        H = torch.from_numpy(poses).to(dev)
        count = None if live is None else torch.full((B,), live, dtype=torch.int64, device=dev)
        n_pose = B * (K if live is None else live)
        leg_a = lambda: PP.eval_frames(H, xyz, nrm, lab, g, inverse="se3", count=count)
        leg_b = lambda: PP.view_non_collision(H, xyz, g, inverse="se3", count=count)
        g2l = PP.se3_inverse(H[0, :args.loop_poses])
        homo = torch.cat([xyz[0], torch.ones(1, N, device=dev)], 0)
        leg_c = lambda: reference_loop(g2l, homo, nrm[0], lab[0], g)
        r = leg_a()
        ok, counts = leg_b()
        assert torch.equal(r.ints[..., :2], counts)
        ref = leg_c()
        got = r.score[0, :args.loop_poses].cpu().numpy()
        want = np.array([float(x["antipodal_score"]) for x in ref])
        for _ in range(3):
            leg_a(); leg_b()
        torch.cuda.synchronize()
        ta, tb, tc = [], [], []
        for i in range(args.repeat):
            for leg in ("ab", "ba")[i % 2]:
                (ta if leg == "a" else tb).append(timed(leg_a if leg == "a" else leg_b, args.inner))
            if i < 3:
                tc.append(timed(leg_c, 1))
        a, b, c = float(np.median(ta)), float(np.median(tb)), float(np.median(tc)) * n_pose / args.loop_poses
        live_rows = torch.arange(K, device=dev).view(1, K) < (count.view(B, 1) if count is not None else K)
        print(json.dumps({
            "B": B, "N": N, "K": K, "poses_per_scene": K if live is None else live,
            "eval_frames_ms": round(a, 4), "eval_frames_min_max_ms": [round(min(ta), 4), round(max(ta), 4)],
            "collision_counts_ms": round(b, 4), "collision_min_max_ms": [round(min(tb), 4), round(max(tb), 4)],
            "ratio_a_over_b": round(a / b, 3),
            "reference_loop_ms_scaled": round(c, 1), "reference_loop_poses_run": args.loop_poses,
            "speedup_over_reference_loop": round(c / a, 1),
            "scored_poses": int(((r.score > 0) & live_rows).sum()), "collision_poses": int((r.collision & live_rows).sum()),
            "max_abs_score_diff_vs_loop": float(np.nanmax(np.abs(got - want)))}))


if __name__ == "__main__":
    main()
