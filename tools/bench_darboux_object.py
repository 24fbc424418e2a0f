#!/usr/bin/env python3
"""Times the curvature model's per-object data on the fixture's object (tests/golden/darboux_object.npz: 5 324 points),
in one process:

  (a) estimate_object_frames              the ordered grid, every point's frame and opposite frame
                                          (s4g_darboux_object_frames_f32)
  (b) grade_object_frames                 both frames of every point over the cloud, 4 x 12 x 3 each
                                          (s4g_darboux_object_grade_f32)
  (c) label_darboux_object                (a) + (b), one object
  (d) label_darboux_object                `--objects` copies of the object in one batch
  (e) the reference-shaped formulation    finger_hand_view with _antipodal_score (data_object_darboux_generator.py:
                                          131-247) restated on the device -- per frame a fp32 inverse, a 4 x N product,
                                          per depth the slab mask and the 12 x 4 x n rolled product, per roll and shift
                                          the boolean masks and sums with their host reads -- run on `--loop-frames`
                                          frames in both directions and scaled to all points; the kd-tree queries and
                                          the eigh of the reference's frame loop are not in it

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


def reference_loop(points, normals, frames, index, cfg, l2ls):
    """finger_hand_view as written (with the two scalars of decision 1), on the device.  points, normals (N, 3); frames
    (F, 3, 3) at the points `index`.  -> the number of positive placements."""
    dev = points.device
    N = points.shape[0]
    homo = torch.cat([points.t(), torch.ones(1, N, device=dev)], 0)
    nrm = normals.t().contiguous()
    L, T = len(cfg.length_search), len(cfg.theta_search_deg)
    hbw, hbs, hht = cfg.half_bottom_width, cfg.half_bottom_space, cfg.half_hand_thickness
    nd = torch.tensor(cfg.neighbor_depth, device=dev)
    left = torch.tensor([[0.0, 1.0, 0.0]], device=dev)
    positive = 0
    for f in range(len(frames)):
        out = torch.zeros(L, T, device=dev)
        Tm = torch.eye(4, device=dev)
        Tm[0:3, 0:3] = frames[f]
        Tm[0:3, 3:4] = homo[0:3, index[f]:index[f] + 1]
        Tm = torch.inverse(Tm)
        lc = torch.matmul(Tm, homo)
        ln = torch.matmul(Tm[0:3, 0:3], nrm)
        for d, dl in enumerate(cfg.length_search):
            cp = (lc[0] < dl + cfg.finger_length) & (lc[0] > dl - cfg.bottom_length)
            if torch.sum(cp) < cfg.num_points_threshold:
                continue
            pts = lc[:, cp]
            allp = torch.matmul(l2ls[d * T:(d + 1) * T].contiguous().view(-1, 4), pts).view(T, 4, -1)[:, 0:3]
            for r in range(T):
                c = allp[r]
                bxy = (c[1] < hbw) & (c[1] > -hbw) & (c[0] < -cfg.back_collision_margin)
                fl = (c[1] < hbw) & (c[1] > hbs)
                fr = (c[1] > -hbw) & (c[1] < -hbs)
                ts, ta = torch.zeros(2, device=dev)
                crn, single = torch.zeros(2, device=dev)
                for dz in cfg.shift_search:
                    zc = (c[2] < hht + dz) & (c[2] > -hht + dz)
                    if torch.sum(bxy & zc) > cfg.back_collision_threshold:
                        continue
                    if torch.sum(zc & (fl | fr)) > cfg.finger_collision_threshold:
                        continue
                    cr = zc & (c[1] < hbs) & (c[1] > -hbs)
                    crn = torch.sum(cr, dtype=torch.float)
                    if crn < cfg.close_region_min_points:
                        continue
                    cn = torch.matmul(l2ls[d * T + r, 0:3, 0:3], ln[:, cp][:, cr])
                    cc = c[:, cr]
                    ly, ry = torch.max(cc[1]), torch.min(cc[1])
                    dep = torch.min((ly - ry) / 3, nd)
                    lt = torch.abs(torch.matmul(left, cn[:, cc[1] > ly - dep]))
                    rt = torch.abs(torch.matmul(-left, cn[:, cc[1] < ry + dep]))
                    single = torch.mean(lt) * torch.mean(rt)
                    ta += single / 3
                    ts += crn / 3
                out[d, r] = torch.min(ts, crn)
        positive += int((out.to(torch.int) > 0).sum())
    return positive


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--loop-frames", type=int, default=48)
    args = ap.parse_args()
    from s4g_release_amd import postprocess as PP
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "darboux_object.npz"))
    cfg = PP.DarbouxObjectConfig()
    one = lambda k: torch.from_numpy(np.ascontiguousarray(fx[k].T[None])).to(dev)   # noqa: E731
    xyz, nrm = one("points"), one("normals")
    N = int(xyz.shape[2])
    B = args.objects
    xyzB, nrmB = xyz.expand(B, -1, -1).contiguous(), nrm.expand(B, -1, -1).contiguous()
    fr = PP.estimate_object_frames(xyz, nrm, config=cfg)
    legs = {"a": lambda: PP.estimate_object_frames(xyz, nrm, config=cfg),
            "b": lambda: PP.grade_object_frames(xyz, nrm, fr.frames, fr.inv_frames, cfg),
            "c": lambda: PP.label_darboux_object(xyz, nrm, cfg),
            "d": lambda: PP.label_darboux_object(xyzB, nrmB, cfg)}
    out = legs["c"]()
    legs["d"]()
    torch.cuda.synchronize()
    nl = min(args.loop_frames, N)
    sel = torch.arange(0, N, N // nl, device=dev)[:nl]
    pts, nn = xyz[0].t().contiguous(), nrm[0].t().contiguous()
    tb = cfg.tables()
    L, T, _ = cfg.shape
    l2ls = torch.eye(4).repeat(L * T, 1, 1)
    l2ls[:, 0, 3] = -tb["depth"].repeat_interleave(T)
    l2ls[:, 1, 1] = l2ls[:, 2, 2] = tb["cos"].repeat(L)
    l2ls[:, 1, 2] = tb["sin"].repeat(L)
    l2ls[:, 2, 1] = -tb["sin"].repeat(L)
    l2ls = l2ls.to(dev)
    both = torch.cat([fr.frames[0, sel], fr.inv_frames[0, sel]])
    idx = torch.cat([sel, sel]).tolist()
    leg_e = lambda: reference_loop(pts, nn, both, idx, cfg, l2ls)                   # noqa: E731
    loop_positive = leg_e()
    ours = int((out.grades.search_score[0, sel] > 0).sum())
    te = float(np.median([timed(leg_e, 1) for _ in range(3)])) * N / nl
    t = {k: [] for k in legs}
    for i in range(args.repeat):
        for k in (list(legs) if i % 2 == 0 else list(legs)[::-1]):
            t[k].append(timed(legs[k], args.inner))
    med = {k: float(np.median(x)) for k, x in t.items()}
    spread = {k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()}
    print(json.dumps({
        "N": N, "rows": 2 * N, "placements_per_row": L * T, "objects": B,
        "positive_placements": int((out.grades.search_score > 0).sum()),
        "estimate_object_frames_ms": round(med["a"], 3), "frames_min_max_ms": spread["a"],
        "grade_object_frames_ms": round(med["b"], 3), "grade_min_max_ms": spread["b"],
        "label_darboux_object_ms": round(med["c"], 3), "label_min_max_ms": spread["c"],
        "label_darboux_object_batch_ms": round(med["d"], 3), "batch_min_max_ms": spread["d"],
        "point_row_transforms_per_second": round(2 * N * N / (med["b"] * 1e-3)),
        "reference_loop_ms_scaled_to_all_points": round(te, 1), "reference_loop_frames_run": nl,
        "loop_positive_vs_ours_on_those_frames": "%d vs %d" % (loop_positive, ours),
        "speedup_of_grading_over_the_loop": round(te / med["b"], 1)}), flush=True)


if __name__ == "__main__":
    main()
