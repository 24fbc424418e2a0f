#!/usr/bin/env python3
"""Times the baselines' evaluation data: `--views` views of `--view-points` points with `--frames` frames each against
dense scenes of `--scene-points` points (the synthetic table-top scene of tools/bench_precomputed_view.py; every view is
another noisy pick of its points with the scene's normals).

  (1) label_eval_view              the whole call: estimate_frames, the view search, close_regions, the scene grade
  (2) grade_eval_view_frames       the view search alone (s4g_eval_view_search_f32), against
      the shipped three-word search  grade_precomputed_baseline_frames on the SAME frames with an all-true mask and a
                                     constant score (s4g_precomputed_baseline_search_f32), timed ALTERNATING
  (3) grade_eval_scene_frames      the scene grade alone (s4g_eval_scene_grade_f32) on the matrices (1) took, compacted to
                                   the front of every view's list, against
      eval_frames' kernel            s4g_eval_frames_f32 on the SAME matrices and counts, timed ALTERNATING
  (4) the reference-shaped loop    finger_hand_view and finger_hand_scene as written (evaluation_data_generator.py:
                                   228-391), one frame after the other on the device with its host reads, run on
                                   `--loop-frames` frames of one view and scaled to all frames of all views

The new kernels do the work of their shipped counterparts plus one counter each (the reach gate in the setup kernel;
the slab count in the first scan): `ratio` = new median / shipped median, and `within_spread` says whether the two sets
of timed calls overlap (max of the faster <= min of the slower does not hold).

Method: one warm-up call per leg, then `--repeat` timed calls per leg between device events; min / median / max per
leg.  One JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_precomputed_view import make_case, timed      # noqa: E402


def stats(ms):
    return {"calls": len(ms), "min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3),
            "max_ms": round(max(ms), 3)}


def compare(new, old):
    return {"ratio": round(float(np.median(new) / np.median(old)), 3),
            "within_spread": not (max(new) < min(old) or max(old) < min(new))}


def reference_loop(points, frames, view_homo, scene_homo, scene_normals, scene_labels, s, l2ls, s2l, bound):
    """finger_hand_view, then finger_hand_scene of a taken placement, one frame after the other.  -> grasps taken."""
    dev = view_homo.device
    L, T = s.shape
    hbw, hbs, hht = s.half_bottom_width, s.half_bottom_space, s.half_hand_thickness
    limit = s.table_height + s.table_collision_offset
    nd = torch.tensor(s.neighbor_depth, device=dev)
    taken = 0
    for f in range(len(points)):
        if torch.mean(torch.abs(frames[f])) < 1e-6:
            continue
        if points[f, 2] + frames[f, 2, 0] * s.finger_length < s.table_height:
            continue
        l2g = torch.eye(4, device=dev)
        l2g[0:3, 0:3] = frames[f]
        l2g[0:3, 3] = points[f]
        corners = torch.bmm(torch.bmm(l2g.unsqueeze(0).expand(L * T, 4, 4).contiguous(), s2l),
                            bound.expand(L * T, -1, -1).contiguous())
        table = (corners[:, 2, :] < limit).any(dim=1)
        g2l = torch.eye(4, device=dev)
        g2l[0:3, 0:3] = frames[f].t()
        g2l[0:3, 3:4] = -torch.matmul(frames[f].t(), points[f].unsqueeze(1))
        lc = torch.matmul(g2l, view_homo)
        best, i = None, 0
        for d, dl in enumerate(s.length_search):
            if best is not None:
                break
            cp = (lc[0] < dl + s.finger_length) & (lc[0] > dl - s.bottom_length)
            if torch.sum(cp) < s.num_points_threshold:
                i += T
                continue
            allp = torch.matmul(l2ls[d * T:(d + 1) * T].contiguous().view(-1, 4), lc[:, cp]).view(T, 4, -1)[:, 0:3]
            for r in range(T):
                if table[i]:
                    i += 1
                    continue
                c = allp[r]
                zc = (c[2] < hht) & (c[2] > -hht)
                if torch.sum((c[1] < hbw) & (c[1] > -hbw) & (c[0] < -s.back_collision_margin) & zc) > s.back_collision_threshold:
                    i += 1
                    continue
                fg = ((c[1] < hbw) & (c[1] > hbs)) | ((c[1] > -hbw) & (c[1] < -hbs))
                if torch.sum(zc & fg) > s.finger_collision_threshold:
                    i += 1
                    continue
                if torch.sum(zc & (c[1] < hbs) & (c[1] > -hbs)) < s.close_region_min_points:
                    i += 1
                    continue
                best = torch.matmul(l2ls[i], g2l)
                break
        if best is None:
            continue
        taken += 1
        lc = torch.matmul(best, scene_homo)
        ln = torch.matmul(best[0:3, 0:3], scene_normals)
        cp = (lc[0] < s.finger_length) & (lc[0] > -s.bottom_length)
        if torch.sum(cp) < s.num_points_threshold:
            continue
        c = lc[:, cp][0:3]
        zc = (c[2] < hht) & (c[2] > -hht)
        if torch.sum((c[1] < hbw) & (c[1] > -hbw) & (c[0] < -s.back_collision_margin) & zc) > s.back_collision_threshold:
            continue
        fg = ((c[1] < hbw) & (c[1] > hbs)) | ((c[1] > -hbw) & (c[1] < -hbs))
        if torch.sum(zc & fg) > s.finger_collision_threshold:
            continue
        cr = zc & (c[1] < hbs) & (c[1] > -hbs)
        if torch.unique(scene_labels[cp][cr], sorted=False).shape[0] > 1:
            continue
        cn, cc = ln[:, cp][:, cr], c[:, cr]
        if cc.shape[1] < s.close_region_min_points:
            continue
        ly, ry = torch.max(cc[1]), torch.min(cc[1])
        depth = torch.min((ly - ry) / 3, nd)
        _ = (torch.mean(torch.abs(cn[1, cc[1] > ly - depth])) * torch.mean(torch.abs(cn[1, cc[1] < ry + depth]))).item()
    return taken


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--scene-points", type=int, default=200000)
    ap.add_argument("--view-points", type=int, default=25600)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--loop-frames", type=int, default=48)
    args = ap.parse_args()
    from s4g_release_amd import _cabi
    from s4g_release_amd import functions as Fn
    from s4g_release_amd import postprocess as PP
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    cfg = PP.EvalDataConfig(grasp_num=args.frames)
    s = cfg.search
    L, T = s.shape
    B = args.views
    sc, _, _ = make_case(5, args.scene_points, 8, PP.PrecomputedBaselineConfig(search=s))
    M = sc["points"].shape[1]
    rng = np.random.default_rng(9)
    pick = np.stack([rng.choice(M, args.view_points) for _ in range(B)])
    view = sc["points"].T[pick].astype(np.float64) + rng.normal(0, 0.002, (B, args.view_points, 3))
    cloud = torch.from_numpy(np.ascontiguousarray(view.transpose(0, 2, 1), dtype=np.float32)).to(dev)
    normals = torch.from_numpy(np.ascontiguousarray(sc["normals"].T[pick].transpose(0, 2, 1), dtype=np.float32)).to(dev)
    scene = torch.from_numpy(sc["points"]).to(dev)[None].expand(B, 3, M).contiguous()
    snrm = torch.from_numpy(sc["normals"]).to(dev)[None].expand(B, 3, M).contiguous()
    slab = torch.from_numpy(sc["labels"].astype(np.int32)).to(dev)[None].expand(B, M).contiguous()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    whole = lambda: PP.label_eval_view(cloud, normals, scene, snrm, slab, cfg, generator=gen)        # noqa: E731
    v = whole()
    torch.cuda.synchronize()
    pts, frm, fcnt = v.frames.points, v.frames.frames, v.frames.frame_count
    live = v.frames.count >= cfg.min_neighbours
    F = pts.shape[1]
    # the shipped search has no `live`: both legs of (2) run on frames whose dead rows hold the zero frame
    frm2 = torch.where(live.view(B, F, 1, 1), frm, torch.zeros((), device=dev)).contiguous()
    ones = torch.ones((B, F, L, T), dtype=torch.float32, device=dev)
    mask = ones > 0
    pb = PP.PrecomputedBaselineConfig(search=s)
    new_view = lambda: PP.grade_eval_view_frames(pts, frm2, cloud, cfg, fcnt)                         # noqa: E731
    old_view = lambda: PP.grade_precomputed_baseline_frames(pts, frm2, mask, ones, cloud, pb, fcnt)   # noqa: E731
    # both legs of (3) grade the SAME rows: the taken placements, compacted to the front of every view's list (a row
    # that was not taken holds the zero matrix, in whose "close region" the other class finds every scene point)
    vi = v.search.valid_index.clamp(min=0).long()
    g2l = torch.gather(v.search.global_to_local, 1, vi.view(B, F, 1, 1).expand(B, F, 4, 4)).contiguous()
    cnt = v.search.count
    taken = torch.arange(F, device=dev).view(1, F) < cnt.view(B, 1)
    new_scene = lambda: PP.grade_eval_scene_frames(g2l, scene, snrm, slab, cfg, cnt)                 # noqa: E731
    e_ints = torch.empty((B, F, 8), dtype=torch.int32, device=dev)
    e_floats = torch.empty((B, F, 5), dtype=torch.float32, device=dev)
    nbytes = int(_cabi.lib().s4g_eval_frames_workspace_bytes(B, M, F))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    p10 = (ctypes.c_float * 10)(s.finger_length, s.bottom_length, s.half_hand_thickness, s.half_bottom_width,
                                s.half_bottom_space, s.back_collision_margin, s.back_collision_threshold,
                                s.finger_collision_threshold, s.close_region_min_points, s.neighbor_depth)

    def old_scene():
        rc = _cabi.lib().s4g_eval_frames_f32(scene.data_ptr(), snrm.data_ptr(), slab.data_ptr(), g2l.data_ptr(), B, M, F,
                                             p10, cnt.data_ptr(), 0, e_ints.data_ptr(), e_floats.data_ptr(),
                                             ws.data_ptr(), nbytes, Fn._stream())
        assert rc == 0
    # the outputs agree at the timed size first
    a, b = new_view(), old_view()
    reach = (a.flags & 8) == 0
    assert torch.equal(a.ints[reach], b.ints[reach]) and torch.equal(a.index[reach], b.best.index[reach])
    t = new_scene()
    old_scene()
    torch.cuda.synchronize()
    assert torch.equal(t.ints[..., 1:4][taken], e_ints[..., 0:3][taken])
    out = {"views": B, "view_points": args.view_points, "scene_points": M, "frames": F,
           "frames_searched": int((a.flags == 0).sum()),
           "frames_past_the_reach_gate_only": int((a.flags == 8).sum()), "grasps": int(taken.sum()),
           "scored": int(((t.stage == 0) & taken).sum())}
    ms = {k: [] for k in ("whole", "view", "view_shipped", "scene", "scene_shipped")}
    for fn in (whole, new_view, old_view, new_scene, old_scene):
        fn()
    torch.cuda.synchronize()
    for _ in range(args.repeat):
        ms["whole"].append(timed(whole))
    for _ in range(args.repeat):
        ms["view"].append(timed(new_view))
        ms["view_shipped"].append(timed(old_view))
    for _ in range(args.repeat):
        ms["scene"].append(timed(new_scene))
        ms["scene_shipped"].append(timed(old_scene))
    out.update({k: stats(x) for k, x in ms.items()})
    out["view_vs_shipped"] = compare(ms["view"], ms["view_shipped"])
    out["scene_vs_shipped"] = compare(ms["scene"], ms["scene_shipped"])
    # (4) the reference-shaped loop on a few frames of view 0
    n = min(args.loop_frames, int(fcnt[0]))
    l2ls = torch.zeros(L * T, 4, 4, device=dev)
    tb = s.tables()
    for d in range(L):
        for r in range(T):
            m = torch.eye(4)
            m[0, 3] = -tb["depth"][d]
            m[1, 1] = m[2, 2] = tb["cos"][r]
            m[1, 2], m[2, 1] = tb["sin"][r], -tb["sin"][r]
            l2ls[d * T + r] = m
    s2l = s.search_to_local().view(L * T, 4, 4).to(dev)
    bound = torch.tensor([[x, y, z, 1.0] for x in (s.finger_length, -s.bottom_length)
                          for y in (s.half_bottom_width, -s.half_bottom_width)
                          for z in (s.half_hand_thickness, -s.half_hand_thickness)], device=dev).t().unsqueeze(0)
    vh = torch.cat([cloud[0], torch.ones(1, cloud.shape[2], device=dev)], 0)
    sh = torch.cat([scene[0], torch.ones(1, M, device=dev)], 0)
    loop = lambda: reference_loop(pts[0, :n], frm2[0, :n], vh, sh, snrm[0], slab[0], s, l2ls, s2l, bound)   # noqa: E731
    loop()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = loop()
    torch.cuda.synchronize()
    per_frame = (time.perf_counter() - t0) * 1e3 / max(n, 1)
    total = int(fcnt.sum())
    out["reference_loop"] = {"frames_run": n, "grasps": got, "ms_per_frame": round(per_frame, 3),
                             "scaled_ms": round(per_frame * total, 1),
                             "speedup_of_whole_call": round(per_frame * total / float(np.median(ms["whole"])), 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
