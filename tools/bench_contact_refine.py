#!/usr/bin/env python3
"""Times the refine and reduce stages of the contact-object pipeline, in one process, on the fixture's object
(tests/golden/contact_pairs.npz: 5 324 points, 3 874 frames) and on `--objects` synthetic objects of `--points` points
with `--frames` frames each:

  (a) refine_contact_frames              s4g_contact_refine_f32: the three-word sweep, the finish, the compaction
  (b) grade_contact_frames               s4g_contact_search_f32 on the same rows with zero labels and
                                         back_collision_margin 0: the five-word sweep refine could call instead;
                                         (a) and (b) timed alternating
  (c) the reference-shaped formulation   check_single_collision (refine_contact_object.py:71-97) restated on the device
                                         -- per frame a 4 x M product, nine sets of boolean masks and their host reads
                                         -- run on `--loop-frames` live frames and scaled to all live frames
  (d) reduce_contact_frames              and its three parts: the CSR of the filtered frames by point (torch), the
                                         neighbour search (s4g_match_knn_f32), the fold (s4g_contact_reduce_i32)
  (e) the script's reduce loop           smooth_contact_object.py:61-89 in numpy on the host (a float64 brute-force
                                         search for the querying points in place of the kd-tree)

Method: warm-up, then `--repeat` rounds of `--inner` calls between device events, the legs in alternating order; the
median and the spread (min, max) per leg.  One JSON line per data set."""
import argparse
import json
import os
import sys
import time

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


def reference_loop(points, g2l, cfg):
    """check_single_collision per frame, as written, on the device -> the kept count."""
    M = points.shape[0]
    homo = torch.cat([points.t(), torch.ones(1, M, device=points.device)], 0)
    hht, hbs, hbw = cfg.half_hand_thickness, cfg.half_bottom_space, cfg.half_bottom_width
    kept = 0
    for i in range(g2l.shape[0]):
        lc = g2l[i] @ homo
        ok = True
        for dz in cfg.height_search:
            zb = (lc[2] < hht + dz) & (lc[2] > -hht + dz)
            for dy in cfg.width_search:
                yb = (lc[1] < hbs + dy) & (lc[1] > -hbs + dy)
                ay = torch.abs(lc[1] + dy)
                yc = (ay > hbs) & (ay < hbw)
                for dx in cfg.length_search:
                    xb = (lc[0] > -cfg.bottom_length + dx) & (lc[0] < cfg.finger_length + dx)
                    if (zb & xb & yc).sum() > cfg.collision_threshold:
                        ok = False
                        break
                    close = xb & zb & yb
                    if close.sum() < cfg.min_search_score:
                        ok = False
                        break
                    if lc[0, close].min() < 0:
                        ok = False
                        break
                if not ok:
                    break
            if not ok:
                break
        kept += int(ok)
    return kept


def host_reduce_loop(cloud, fpi, search, cfg):
    """smooth_contact_object.py:37-89 on the host -> the output frame count."""
    valid = np.nonzero(search > cfg.min_search_score)[0]
    fpi = fpi[valid]
    N = len(cloud)
    num = np.zeros(N, np.int64)
    out = 0
    fpp = cfg.frame_per_point
    for i in range(N):
        pf = np.nonzero(fpi == i)[0]
        if len(pf) > fpp:
            new = pf[0:fpp - num[i]]
            out += len(new)
            num[i] += len(new)
            rest = pf[fpp:]
            if len(rest) > cfg.min_rest:
                d2 = ((cloud - cloud[i]) ** 2).sum(1)
                idx = np.nonzero(d2 < cfg.radius ** 2)[0]
                idx = idx[np.lexsort((idx, d2[idx]))][:cfg.max_nn]
                for n in idx:
                    if (n < i and num[n] < fpp) or (n > i and num[n] < cfg.max_neighbor_frame):
                        num[n] += 1
                        out += 1
        elif len(pf) > 0:
            added = min(fpp - num[i], len(pf))
            out += added
            num[i] += added
    return out


def synthetic(B, M, F, seed, dev):
    """B objects: M points on a 6 x 4 x 3 cm box surface, F rigid frames whose origins lie near it."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    P = (torch.rand((B, 3, M), generator=g) - 0.5) * torch.tensor([0.06, 0.04, 0.03]).view(1, 3, 1)
    face = torch.randint(0, 3, (B, 1, M), generator=g)
    side = torch.where(torch.rand((B, 1, M), generator=g) < 0.5, -0.5, 0.5) * torch.tensor([0.06, 0.04, 0.03]).view(1, 3, 1)
    P = torch.where(torch.arange(3).view(1, 3, 1) == face, side, P)
    q = torch.randn((B, F, 4), generator=g)
    q = q / q.norm(dim=2, keepdim=True)
    w, x, y, z = q.unbind(2)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 2).view(B, F, 3, 3)
    G = torch.zeros((B, F, 4, 4))
    G[:, :, :3, :3] = R
    G[:, :, :3, 3] = (torch.rand((B, F, 3), generator=g) - 0.3) * 0.04
    G[:, :, 3, 3] = 1
    search = torch.randint(40, 400, (B, F), generator=g).float()
    fpi = torch.randint(0, M, (B, F), generator=g).int()
    fpi[:, :F // 4] = fpi[:, :F // 4] % max(M // 200, 1)              # a share of the frames crowd on few points
    return P.contiguous().to(dev), G.to(dev), search.to(dev), fpi.to(dev)


def measure(name, xyz, g2l, search, fpi, args, loop, reduce_refined):
    from s4g_release_amd import contact_object as CO
    from s4g_release_amd import postprocess as PP
    dev = xyz.device
    B, _, M = xyz.shape
    F = g2l.shape[1]
    rcfg, dcfg = CO.ContactRefineConfig(), CO.ContactReduceConfig()
    scfg = PP.ContactSearchConfig(width_search=rcfg.width_search, height_search=rcfg.height_search,
                                  length_search=rcfg.length_search, back_collision_margin=0.0)
    zero = torch.zeros((B, M), dtype=torch.int32, device=dev)
    live = search > rcfg.min_search_score
    # the same rows for both sweeps: the live ones in front, the count in frame_count
    order = torch.argsort((~live).to(torch.int8), dim=1, stable=True)
    g_live = torch.gather(g2l, 1, order[:, :, None, None].expand(-1, -1, 4, 4)).contiguous()
    s_live = torch.gather(search, 1, order)
    n_live = live.sum(1)
    ref = CO.refine_contact_frames(xyz, g2l, search, rcfg)
    # the reduce stage's input: the refined list, or (random frames of a synthetic box almost all collide) the list as given
    score = ref.search_score if reduce_refined else search
    cap = min(F, M * dcfg.frame_per_point)
    csr = CO._frames_of_points(fpi, score, dcfg, M, None, None)
    knn = CO._neighbours(xyz, None, dcfg)
    legs = {"refine": lambda: CO.refine_contact_frames(xyz, g_live, s_live, rcfg, frame_count=n_live),
            "grade": lambda: PP.grade_contact_frames(g_live, xyz, zero, scfg, frame_count=n_live),
            "reduce": lambda: CO.reduce_contact_frames(xyz, fpi, score, dcfg),
            "reduce_csr": lambda: CO._frames_of_points(fpi, score, dcfg, M, None, None),
            "reduce_knn": lambda: CO._neighbours(xyz, None, dcfg),
            "reduce_fold": lambda: CO._fold(csr[0], csr[1], csr[2], knn, None, dcfg, cap)}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for i in range(args.repeat):
        for k in (list(legs) if i % 2 == 0 else list(legs)[::-1]):
            t[k].append(timed(legs[k], args.inner))
    res = {"data": name, "objects": B, "points": M, "frames": F, "live": int(n_live.sum()),
           "kept": int(ref.kept_count.sum()), "reduced": int(legs["reduce"]().count.sum())}
    for k, x in t.items():
        res[k + "_ms"] = round(float(np.median(x)), 3)
        res[k + "_min_max_ms"] = [round(min(x), 3), round(max(x), 3)]
    res["point_frame_transforms_per_second"] = round(int(n_live.sum()) * M / (res["refine_ms"] * 1e-3))
    if loop:
        nl = min(args.loop_frames, int(n_live[0]))
        pts = xyz[0].t().contiguous()
        leg = lambda: reference_loop(pts, g_live[0, :nl], rcfg)                      # noqa: E731
        ours = int(CO.refine_contact_frames(xyz[:1], g_live[:1, :nl], s_live[:1, :nl], rcfg).kept_count[0])
        kept = leg()
        tl = float(np.median([timed(leg, 1) for _ in range(3)])) * int(n_live.sum()) / nl
        res.update(reference_loop_ms_scaled_to_live_frames=round(tl, 1), reference_loop_frames_run=nl,
                   loop_kept_vs_ours_on_those_frames="%d vs %d" % (kept, ours),
                   speedup_of_refine_over_the_loop=round(tl / res["refine_ms"], 1))
        cloud = xyz[0].t().double().cpu().numpy()
        h_fpi, h_score = fpi[0].cpu().numpy(), score[0].cpu().numpy()
        t0 = time.perf_counter()
        n = host_reduce_loop(cloud, h_fpi, h_score, dcfg)
        th = (time.perf_counter() - t0) * 1e3
        one = int(CO.reduce_contact_frames(xyz[:1], fpi[:1], score[:1], dcfg).count[0])
        res.update(host_reduce_loop_ms_one_object=round(th, 1), host_loop_frames_vs_ours="%d vs %d" % (n, one))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=16)
    ap.add_argument("--points", type=int, default=30000)
    ap.add_argument("--frames", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--loop-frames", type=int, default=48)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "contact_pairs.npz"))
    one = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)               # noqa: E731
    measure("fixture", one(fx["points"].T[None]), one(fx["global_to_local"][None]), one(fx["search_score"][None]),
            one(fx["frame_point_index"][None]), args, loop=True, reduce_refined=True)
    xyz, g2l, search, fpi = synthetic(args.objects, args.points, args.frames, 1, dev)
    measure("synthetic", xyz, g2l, search, fpi, args, loop=True, reduce_refined=False)


if __name__ == "__main__":
    main()
