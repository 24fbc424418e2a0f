#!/usr/bin/env python3
"""Times the contact model's per-object data on the fixture's object (tests/golden/contact_pairs.npz: 5 324 points),
in one process:

  (a) contact_pairs                       the N x N antipodal test and the ordered list (s4g_contact_pairs_f32)
  (b) grade_contact_pairs                 every listed pair over the cloud, the kept frames and their nearest points
                                          (s4g_contact_pair_grade_f32)
  (c) label_contact_object                (a) + (b), one object
  (d) label_contact_object                `--objects` copies of the object in one batch
  (e) the reference-shaped formulation    check_collision (data_object_contact_point_generator.py:167-221) restated on
                                          the device -- per pair a 4 x N product, the 12 x 4 x N rolled product, the
                                          boolean masks and sums with their host reads -- run on `--loop-pairs` pairs and
                                          scaled to the whole list; the pair search and the kd-tree queries of the
                                          reference are not in it

Method: warm-up, then `--repeat` rounds of `--inner` calls between device events, the legs in alternating order; the
median and the spread per leg.  One JSON line."""
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


def reference_loop(points, pairs, cfg, l2ls):
    """_estimate_grasp_quality's frames (:137-152) and check_collision per pair, as written, on the device."""
    N = points.shape[0]
    homo = torch.cat([points.t(), torch.ones(1, N, device=points.device)], 0)
    ey = torch.tensor([[0.0, 1.0, 0.0]], device=points.device)
    y = points[pairs[:, 1]] - points[pairs[:, 0]]
    y = y / y.norm(dim=1, keepdim=True)
    x = ey - (ey * y).sum(1, keepdim=True) * y
    x = x / x.norm(dim=1, keepdim=True)
    z = torch.cross(x, y, dim=1)
    fr = torch.zeros(len(pairs), 4, 4, device=points.device)
    fr[:, :3, 0], fr[:, :3, 1], fr[:, :3, 2] = x, y, z
    fr[:, :3, 3] = (points[pairs[:, 0]] + points[pairs[:, 1]]) / 2
    fr[:, 3, 3] = 1
    T = torch.inverse(fr)
    hbs, hbw, hht = cfg.half_bottom_space, cfg.half_bottom_width, cfg.half_hand_thickness
    frames = 0
    for i in range(len(pairs)):
        lc = torch.matmul(T[i], homo)
        cp = (lc[1] < hbs) & (lc[1] > -hbs)
        if torch.sum(cp) < cfg.min_points:
            continue
        fp = ((lc[1] < hbw) & (lc[1] > hbs)) | ((lc[1] > -hbw) & (lc[1] < -hbs))
        bp = fp | cp
        lsc = torch.matmul(l2ls, lc.unsqueeze(0))
        for d in range(l2ls.shape[0]):
            c = lsc[d]
            bx = (c[0] < cfg.back_collision_margin) & (c[0] > -cfg.bottom_length)
            fx = (c[0] > cfg.back_collision_margin) & (c[0] < cfg.finger_length)
            acc = torch.zeros(1, device=points.device)
            for dw in cfg.width_shift:
                crn = torch.zeros(1, device=points.device)
                zc = (c[2] < hht + dw) & (c[2] > -hht + dw)
                if torch.sum(bx & zc & bp) > cfg.back_threshold:
                    continue
                if torch.sum(fx & zc & fp) > cfg.finger_threshold:
                    continue
                crn = torch.sum(fx & cp & zc, dtype=torch.float)
                if crn < cfg.min_points:
                    continue
                acc += crn / 3
            if acc < cfg.min_points or crn < cfg.min_points:
                continue
            frames += 1
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--loop-pairs", type=int, default=48)
    args = ap.parse_args()
    from s4g_release_amd import postprocess as PP
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "contact_pairs.npz"))
    cfg = PP.ContactPairConfig()
    one = lambda k: torch.from_numpy(np.ascontiguousarray(fx[k].T[None])).to(dev)   # noqa: E731
    xyz, nrm = one("points"), one("normals")
    B = args.objects
    xyzB, nrmB = xyz.expand(B, -1, -1).contiguous(), nrm.expand(B, -1, -1).contiguous()
    K = len(fx["pair_row"])
    F = 5 * K
    prs = PP.contact_pairs(xyz, nrm, cfg, max_pairs=K)
    legs = {"a": lambda: PP.contact_pairs(xyz, nrm, cfg, max_pairs=K),
            "b": lambda: PP.grade_contact_pairs(xyz, prs, cfg, max_frames=F),
            "c": lambda: PP.label_contact_object(xyz, nrm, cfg, max_pairs=K, max_frames=F),
            "d": lambda: PP.label_contact_object(xyzB, nrmB, cfg, max_pairs=K, max_frames=F)}
    out = legs["c"]()
    legs["d"]()
    torch.cuda.synchronize()
    nl = min(args.loop_pairs, K)
    sel = torch.arange(0, K, K // nl, device=dev)[:nl]
    pts = xyz[0].t().contiguous()
    l2ls = cfg.local_to_local_search().to(dev)
    leg_e = lambda: reference_loop(pts, prs.pairs[0, sel].long(), cfg, l2ls)        # noqa: E731
    loop_frames = leg_e()
    ours = int(out.grades.valid_i32[0, sel].sum())
    te = float(np.median([timed(leg_e, 1) for _ in range(3)])) * K / nl
    t = {k: [] for k in legs}
    for i in range(args.repeat):
        for k in (list(legs) if i % 2 == 0 else list(legs)[::-1]):
            t[k].append(timed(legs[k], args.inner))
    med = {k: float(np.median(x)) for k, x in t.items()}
    spread = {k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()}
    print(json.dumps({
        "N": int(xyz.shape[2]), "pairs": int(out.pairs.count[0]), "frames": int(out.frame_count[0]), "objects": B,
        "contact_pairs_ms": round(med["a"], 3), "contact_pairs_min_max_ms": spread["a"],
        "grade_contact_pairs_ms": round(med["b"], 3), "grade_min_max_ms": spread["b"],
        "label_contact_object_ms": round(med["c"], 3), "label_min_max_ms": spread["c"],
        "label_contact_object_batch_ms": round(med["d"], 3), "batch_min_max_ms": spread["d"],
        "point_pair_transforms_per_second": round(K * xyz.shape[2] / (med["b"] * 1e-3)),
        "reference_loop_ms_scaled_to_all_pairs": round(te, 1), "reference_loop_pairs_run": nl,
        "loop_frames_vs_ours_on_those_pairs": "%d vs %d" % (loop_frames, ours),
        "speedup_of_grading_over_the_loop": round(te / med["b"], 1)}), flush=True)


if __name__ == "__main__":
    main()
