#!/usr/bin/env python3
"""Times the Darboux frame estimation (`postprocess.estimate_frames`) and the whole labelling call built on it
(`postprocess.label_view`), in one process:

  (a) estimate_frames                     the kernel alone, every point a frame (the rows are given: no index selection)
  (b) label_view                          index selection + estimate_frames + grade_local_search, the view graded
                                          against itself with labels by object (the reference's eval mode)
  (c) the reference-shaped formulation    the per-point loop of torch_single_view_point_cloud.py:103-133 restated on the
                                          device (a distance row, a host read of k, `torch.linalg.eigh` per frame), run
                                          on `--loop-frames` frames of one scene and scaled to B * F

Shape: `--scenes` scenes of `--points` points: the objects of the fixture's scene (tests/golden/darboux.npz, the points
above the sample region) repeated on a 0.6 m pitch with a 0.3 mm jitter, so that the neighbour counts stay those of the
fixture's sampling density; every point is above the sample region and therefore a frame.  Method: warm-up, then
`--repeat` rounds of `--inner` calls between device events; the median and the spread per leg.  One JSON line."""
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


def reference_loop(xyz, normals, index, radius):
    """_estimate_frame (:116-133) per frame, as written: one host read for k."""
    pts, nrm = xyz.t().contiguous(), normals.t().contiguous().double()
    eye = torch.eye(3, dtype=torch.float64, device=xyz.device)
    out = []
    for i in index:
        idx = torch.nonzero(((pts - pts[i]) ** 2).sum(1) < radius * radius)[:, 0]
        if idx.shape[0] < 5:
            out.append(eye)
            continue
        n = nrm[i:i + 1]
        M = eye - n.t() @ n
        c = torch.mean(M @ nrm[idx].t(), dim=1, keepdim=True)
        d = nrm[idx].t() - c
        w, v = torch.linalg.eigh(d @ d.t())
        minor = v[:, 0] - (v[:, 0] @ n.t()) * n[0]
        minor = minor / torch.linalg.norm(minor)
        out.append(torch.stack([-n[0], -torch.linalg.cross(minor, n[0]), minor], 1))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--points", type=int, default=25600)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=48)
    args = ap.parse_args()
    from s4g_release_amd import postprocess as PP
    from tests import darboux_ref as DR
    from tests import golden_util as GU
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    fx = GU.load("darboux.npz")
    radius = float(fx["radius"][0])
    B, N = args.scenes, args.points
    # (2 mm clear of the sample region: the jitter must not move a point below it)
    up = np.nonzero((fx["cloud"][2] > float(fx["sample_region"][0]) + 0.002) & (fx["labels"] != 4))[0]
    copies = -(-N // len(up))
    side = int(np.ceil(np.sqrt(copies)))
    rng = np.random.default_rng(B)
    clouds, nrms, labs = [], [], []
    for b in range(B):
        off = np.array([[0.6 * (c % side), 0.6 * (c // side), 0.0] for c in range(copies)]).T
        cl = (fx["cloud"][:, up][:, None, :] + off[:, :, None]).reshape(3, -1)
        o = rng.permutation(cl.shape[1])[:N]
        clouds.append(cl[:, o] + rng.normal(0, 3e-4, (3, N)))
        nrms.append(np.tile(fx["normals"][:, up], (1, copies))[:, o])
        labs.append(np.tile(fx["labels"][up], copies)[o])
    xyz = torch.from_numpy(np.stack(clouds).astype(np.float32)).to(dev)
    nrm = torch.from_numpy(np.stack(nrms)).to(dev)
    lab = torch.from_numpy(np.stack(labs).astype(np.int32)).to(dev)
    index = torch.arange(N, dtype=torch.int32, device=dev).expand(B, N).contiguous()
    leg_a = lambda: PP.estimate_frames(xyz, nrm, index, None, radius)
    leg_b = lambda: PP.label_view(xyz, nrm, xyz, nrm, lab, radius=radius)
    d = leg_a()
    v = leg_b()
    assert int(v.darboux.frame_count.min()) == N
    torch.cuda.synchronize()
    nf = min(args.loop_frames, N)
    pick = torch.arange(nf, device=dev)
    leg_c = lambda: reference_loop(xyz[0], nrm[0], pick, radius)
    ref = leg_c().cpu().numpy()
    got = d.frames[0, :nf].cpu().numpy()
    loop_err = float(DR.flip_distance(got, ref)[d.estimated[0, :nf].cpu().numpy()].max())
    tc = float(np.median([timed(leg_c, 1) for _ in range(2)])) * B * N / nf
    ta, tb = [], []
    for i in range(args.repeat):
        for leg in ("ab", "ba")[i % 2]:
            (ta if leg == "a" else tb).append(timed(leg_a if leg == "a" else leg_b, args.inner))
    a, b = float(np.median(ta)), float(np.median(tb))
    k = d.count.float()
    print(json.dumps({
        "B": B, "N": N, "F": N, "radius": radius,
        "estimate_frames_ms": round(a, 3), "estimate_frames_min_max_ms": [round(min(ta), 3), round(max(ta), 3)],
        "label_view_ms": round(b, 3), "label_view_min_max_ms": [round(min(tb), 3), round(max(tb), 3)],
        "estimation_share_of_label_view": round(a / b, 4),
        "frames_per_second": round(B * N / (a * 1e-3)),
        "reference_loop_ms_scaled": round(tc, 1), "reference_loop_frames_run": nf,
        "speedup_over_the_loop": round(tc / a, 1), "largest_distance_from_the_loop": loop_err,
        "neighbours_median_max": [float(k.median()), float(k.max())],
        "estimated": int(d.estimated.sum()), "degenerate": int(d.degenerate.sum()),
        "valid_frames": int(v.search.count.sum())}), flush=True)


if __name__ == "__main__":
    main()
