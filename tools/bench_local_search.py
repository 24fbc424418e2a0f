#!/usr/bin/env python3
"""Times the local grasp search (`postprocess.grade_local_search`) against the two routes that existed before it, in one
process:

  (a) grade_local_search                  the new call
  (b) eval_frames on the composed poses   [R | p] @ LOCAL_SEARCH_TO_LOCAL for the L * T placements of every frame,
                                          inverse="se3" (the poses are formed once, outside the timing)
  (c) the reference-shaped formulation    the per-frame torch loop of torch_single_view_point_cloud.py:243-358 restated
                                          here on the device (boolean-mask compactions, torch.unique, a host read per
                                          comparison), run on `--loop-frames` frames of one scene and scaled to B * F

Shape: B scenes of `--points` points (the fixture's table-top scene, tests/golden/local_search.npz, resampled with a
0.3 mm jitter) and `--frames` frames: the fixture's frames repeated with a 2 mm jitter ("on the boxes") and, for one
scene, the same frames moved by up to `--spread` metres across the table ("spread": most of them away from every
object, as the sampled points of a sparse view are).  Method: warm-up, then `--repeat` rounds in which legs (a) and (b)
run in alternating order; the median and the spread per leg, device events around `--inner` calls.  Also prints the
fraction of (point, frame) pairs that pass the cull and reach the L * T placement body.  One JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def reference_loop(pts, frm, homo, normals, labels, cfg, tb, S):
    """finger_hand (:243-358) per frame, as written: one host read per `if`."""
    L, T = cfg.shape
    out = []
    nd = torch.tensor(cfg.neighbor_depth, device=homo.device)
    corners = torch.tensor([[x, y, z, 1.0] for x in (cfg.finger_length, -cfg.bottom_length)
                            for y in (cfg.half_bottom_width, -cfg.half_bottom_width)
                            for z in (cfg.half_hand_thickness, -cfg.half_hand_thickness)], device=homo.device).t()
    hbw, hbs, hht = cfg.half_bottom_width, cfg.half_bottom_space, cfg.half_hand_thickness
    for f in range(len(pts)):
        score = torch.zeros(L, T, device=homo.device)
        search = torch.zeros(L, T, dtype=torch.int, device=homo.device)
        frame, point = frm[f], pts[f]
        if torch.mean(torch.abs(frame)) < 1e-6 or point[2] + frame[2, 0] * cfg.finger_length < cfg.table_height:
            out.append((search, score))
            continue
        H = torch.eye(4, device=homo.device)
        H[:3, :3], H[:3, 3] = frame, point
        table = (torch.matmul(torch.matmul(H, S.view(L * T, 4, 4)), corners)[:, 2] <
                 cfg.table_height + cfg.table_collision_offset).any(1)
        G = torch.eye(4, device=homo.device)
        G[:3, :3] = frame.t()
        G[:3, 3] = -frame.t() @ point
        local = torch.matmul(G, homo)
        ln = torch.matmul(G[:3, :3], normals)
        for d, dl in enumerate(cfg.length_search):
            cp = (local[0] < dl + cfg.finger_length) & (local[0] > dl - cfg.bottom_length)
            if torch.sum(cp) < cfg.num_points_threshold:
                continue
            q = local[:3, cp]
            for t in range(T):
                if table[d * T + t]:
                    continue
                c, sn = tb["cos"][t], tb["sin"][t]
                x, y, z = q[0] - dl, c * q[1] + sn * q[2], -sn * q[1] + c * q[2]
                zin = (z < hht) & (z > -hht)
                if torch.sum((y < hbw) & (y > -hbw) & (x < -cfg.back_collision_margin) & zin) > cfg.back_collision_threshold:
                    continue
                if torch.sum(zin & (((y < hbw) & (y > hbs)) | ((y > -hbw) & (y < -hbs)))) > cfg.finger_collision_threshold:
                    continue
                cr = zin & (y < hbs) & (y > -hbs)
                n = torch.sum(cr)
                if n < cfg.close_region_min_points:
                    continue
                if torch.unique(labels[cp][cr], sorted=False).shape[0] > 1:
                    continue
                search[d, t] = n
                ny = (c * ln[1, cp] + sn * ln[2, cp])[cr]
                cy = y[cr]
                ly, ry = torch.max(cy), torch.min(cy)
                dep = torch.min((ly - ry) / 3, nd)
                score[d, t] = torch.abs(ny[cy > ly - dep]).mean() * torch.abs(ny[cy < ry + dep]).mean()
        out.append((search, score))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=32)
    ap.add_argument("--spread", type=float, default=0.15)
    args = ap.parse_args()
    from s4g_release_amd import postprocess as PP
    from tests import golden_util as GU
    from tests import local_search_ref as LR
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    fx = GU.load("local_search.npz")
    cfg = PP.LocalSearchConfig()
    L, T = cfg.shape
    g = PP.GripperConfig(half_bottom_width=cfg.half_bottom_width, bottom_length=cfg.bottom_length,
                         finger_width=cfg.finger_width, half_hand_thickness=cfg.half_hand_thickness,
                         finger_length=cfg.finger_length, back_collision_margin=cfg.back_collision_margin,
                         back_collision_threshold=cfg.back_collision_threshold,
                         finger_collision_threshold=cfg.finger_collision_threshold,
                         close_region_min_points=cfg.close_region_min_points, neighbor_depth=cfg.neighbor_depth)
    tabs = {k: v.to(dev) for k, v in cfg.tables().items()}
    S = cfg.search_to_local().to(dev)
    cases = [(B, "on the boxes") for B in args.scenes] + [(1, "spread")]
    for B, where in cases:
        rng = np.random.default_rng(B)
        N, F = args.points, args.frames
        idx = rng.integers(0, fx["cloud"].shape[1], (B, N))
        xyz = torch.from_numpy((np.stack([fx["cloud"][:, i] for i in idx])
                                + rng.normal(0, 3e-4, (B, 3, N))).astype(np.float32)).to(dev)
        nrm = torch.from_numpy(np.stack([fx["normals"][:, i] for i in idx])).to(dev)
        lab = torch.from_numpy(np.stack([fx["labels"][i] for i in idx])).to(dev)
        fi = rng.integers(0, len(fx["points"]), (B, F))
        origin = fx["points"][fi] + rng.uniform(-0.002, 0.002, (B, F, 3))
        if where == "spread":
            origin[..., :2] += rng.uniform(-args.spread, args.spread, (B, F, 2))
        pts = torch.from_numpy(origin.astype(np.float32)).to(dev)
        frm = torch.from_numpy(fx["frames"][fi]).to(dev)
        leg_a = lambda: PP.grade_local_search(pts, frm, xyz, nrm, lab, cfg)
        r = leg_a()
        poses = r.frames_of(torch.arange(F, device=dev).expand(B, F)).reshape(B, F * L * T, 4, 4).contiguous()
        leg_b = lambda: PP.eval_frames(poses, xyz, nrm, lab, g, inverse="se3")
        leg_b()
        # culled fraction, from the frames' own matrices (one scene): points inside the slab union and the cylinder
        Rm, p0 = frm[0].double(), pts[0].double()
        sub = xyz[0, :, ::16].double()
        loc = torch.einsum("fji,jn->fin", Rm, sub) - torch.einsum("fji,fj->fi", Rm, p0).unsqueeze(-1)
        lo = min(cfg.length_search) - cfg.bottom_length
        hi = max(cfg.length_search) + cfg.finger_length
        body = ((loc[:, 0] > lo) & (loc[:, 0] < hi)
                & (loc[:, 1] ** 2 + loc[:, 2] ** 2 < cfg.half_bottom_width ** 2 + cfg.half_hand_thickness ** 2))
        del loc
        for _ in range(2):
            leg_a(); leg_b()
        torch.cuda.synchronize()
        tc = None
        if B == 1 and args.loop_frames > 0:
            homo = torch.cat([xyz[0], torch.ones(1, N, device=dev)], 0)
            nf = min(args.loop_frames, F)
            leg_c = lambda: reference_loop(pts[0, :nf], frm[0, :nf], homo, nrm[0], lab[0], cfg, tabs, S)
            ref = leg_c()
            want = torch.stack([x[0] for x in ref])
            loop_diff = int((want != r.search_score[0, :nf]).sum())
            tc = float(np.median([timed(leg_c, 1) for _ in range(2)])) * F / nf
        ta, tb = [], []
        for i in range(args.repeat):
            for leg in ("ab", "ba")[i % 2]:
                (ta if leg == "a" else tb).append(timed(leg_a if leg == "a" else leg_b, args.inner))
        a, b = float(np.median(ta)), float(np.median(tb))
        print(json.dumps({
            "B": B, "N": N, "F": F, "placements": L * T, "frames": where,
            "local_search_ms": round(a, 3), "local_search_min_max_ms": [round(min(ta), 3), round(max(ta), 3)],
            "eval_frames_route_ms": round(b, 3), "eval_route_min_max_ms": [round(min(tb), 3), round(max(tb), 3)],
            "speedup": round(b / a, 2), "fraction_reaching_the_body": round(float(body.float().mean()), 5),
            "reference_loop_ms_scaled": None if tc is None else round(tc, 1),
            "reference_loop_frames_run": None if tc is None else min(args.loop_frames, F),
            "search_scores_differing_from_the_loop": None if tc is None else loop_diff,
            "valid_frames": int(r.count.sum()), "scored_placements": int((r.search_score > 0).sum())}), flush=True)


if __name__ == "__main__":
    main()
