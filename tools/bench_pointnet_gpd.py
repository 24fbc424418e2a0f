#!/usr/bin/env python3
"""Times the PointNetGPD classifier on the close-region point sets, in one process:

  (a) baselines.FusedPointNetGPD                csrc/pointnet_gpd.hip
  (b) baselines.PointNetGPDClassifier in torch  the reference-shaped module on the same device with the same weights,
                                                fp32, after its own warm-up, `--torch-batch` sets per forward (its
                                                1024-wide per-point activations take 4 MB per set of 1 024 points)

Cases (`--cases`):
  packed B N F   every frame of `postprocess.close_regions` on the synthetic scenes of tools/bench_close_region.py, each
                 set whole and at its true size (leg (a) only: the torch module takes sets of one size);
  dense G n      G sets of n points, uniform in the box of a real close region: both legs.
Weights: tests/pointnet_gpd_ref.hashed_state(3) with hashed running statistics.  Method: warm-up, then `--repeat` timings
of `--inner` calls between device events; the median and the spread.  `mfma_tf_issued` counts the fp16 MFMA work the
kernels issue (three products per MAC; whole 32-row blocks of the tiles, whole 32-set blocks of the per-set layers)
over the time of the whole call, to be held against the calibrated loop ceiling of profiles/r05_mfma_ceiling.md
(1 248 TF).  `agreement` is the largest distance of (a) from (b) over the logits' scale.  One JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_close_region import timed  # noqa: E402

MFMA_FLOP = 2 * 32 * 32 * 16
CEILING_TF = 1248.0
BLOCK_MFMA = 2 * 3 * (4 * 4 + 32 * 8)            # per 32 points: two trunks, 64 -> 128 and 128 -> 1024
SETS32_MFMA = 2 * 3 * (16 * 64 + 8 * 32)         # per 32 sets: two heads, 1024 -> 512 and 512 -> 256


def issued_flop(sizes):
    """sizes: the scored sets' point counts (numpy)."""
    blocks = int(((sizes + 31) // 32).sum())
    return (blocks * BLOCK_MFMA + ((len(sizes) + 31) // 32) * SETS32_MFMA) * MFMA_FLOP


def regions_of(dev, B, N, F, points_per_frame):
    from s4g_release_amd import postprocess as PP
    from tests import close_region_ref as CR
    fx = CR.load_fixture()
    base = fx["baseline_frame"][fx["valid"]]
    rng = np.random.default_rng(B)
    idx = rng.integers(0, fx["cloud"].shape[1], (B, N))
    xyz = torch.from_numpy((np.stack([fx["cloud"][:, i] for i in idx]) + rng.normal(0, 3e-4, (B, 3, N))).astype(np.float32)).to(dev)
    nrm = torch.from_numpy(np.stack([fx["normals"][:, i] for i in idx])).to(dev)
    G = base[rng.integers(0, len(base), (B, F))].copy()
    G[..., :3, 3] += rng.uniform(-0.002, 0.002, (B, F, 3)).astype(np.float32)
    r = PP.close_regions(torch.from_numpy(G).to(dev), xyz, nrm, PP.LocalSearchConfig(), capacity=F * points_per_frame)
    torch.cuda.synchronize()
    return r


def report(case, sizes, ta, tb=None, agreement=None):
    a = float(np.median(ta))
    pts = int(sizes.sum())
    out = {"case": case, "sets": int(len(sizes)), "points": pts, "largest_set": int(sizes.max()) if len(sizes) else 0,
           "fused_ms": round(a, 3), "fused_min_max_ms": [round(min(ta), 3), round(max(ta), 3)],
           "fused_points_per_s": round(pts / a * 1e3),
           "mfma_tf_issued": round(issued_flop(sizes) / a * 1e-9, 1),
           "fraction_of_ceiling": round(issued_flop(sizes) / a * 1e-9 / CEILING_TF, 3)}
    if tb is not None:
        b = float(np.median(tb))
        out.update({"torch_ms": round(b, 3), "torch_min_max_ms": [round(min(tb), 3), round(max(tb), 3)],
                    "torch_points_per_s": round(pts / b * 1e3), "torch_over_fused": round(b / a, 2),
                    "agreement": agreement})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["packed", "16", "200000", "512", "packed", "1", "25600", "512",
                                                   "dense", "8192", "1024"])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--torch-batch", type=int, default=256)
    ap.add_argument("--points-per-frame", type=int, default=8192)
    ap.add_argument("--no-torch", action="store_true", help="leg (a) only (for a kernel trace)")
    args = ap.parse_args()
    from s4g_release_amd.baselines import FusedPointNetGPD, PointNetGPDClassifier
    from tests import pointnet_gpd_ref as PR
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    net = PointNetGPDClassifier(3, 3)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in PR.hashed_state(3).items()}, strict=True)
    net = net.to(dev).eval()
    run = FusedPointNetGPD(net)
    run.pack(dev)
    words = list(args.cases)
    while words:
        kind = words.pop(0)
        if kind == "packed":
            B, N, F = (int(words.pop(0)) for _ in range(3))
            r = regions_of(dev, B, N, F, args.points_per_frame)
            leg_a = lambda: run(r.points, offset=r.offset, count=r.count, flags=r.flags, chunk=args.chunk)   # noqa: E731
            for _ in range(3):
                leg_a()
            torch.cuda.synchronize()
            ta = [timed(leg_a, args.inner) for _ in range(args.repeat)]
            cnt, fl = r.count.cpu().numpy().reshape(-1), r.flags.cpu().numpy().reshape(-1)
            report("packed %d x %d x %d" % (B, N, F), cnt[((fl & 1) == 0) & (cnt > 0)].astype(np.int64), ta)
            del r
        elif kind == "dense":
            G, n = int(words.pop(0)), int(words.pop(0))
            gen = torch.Generator(device=dev)
            gen.manual_seed(17)
            lo = torch.tensor([-0.03, 0.0, 0.0], device=dev)[:, None]
            hi = torch.tensor([0.09, 0.08, 0.02], device=dev)[:, None]
            pts = lo + (hi - lo) * torch.rand((G, 3, n), device=dev, generator=gen)
            leg_a = lambda: run(pts, chunk=args.chunk)                                                      # noqa: E731
            sizes = np.full(G, n, np.int64)
            with torch.no_grad():
                def leg_b():
                    return torch.cat([net({"close_region_points": pts[i:i + args.torch_batch]})["grasp_logits"]
                                      for i in range(0, G, args.torch_batch)])
                for _ in range(3):
                    got = leg_a()
                torch.cuda.synchronize()
                ta = [timed(leg_a, args.inner) for _ in range(args.repeat)]
                if args.no_torch:
                    report("dense %d x %d" % (G, n), sizes, ta)
                    continue
                for _ in range(2):
                    ref = leg_b()
                torch.cuda.synchronize()
                agreement = float((got - ref).abs().max() / ref.abs().max())
                tb = [timed(leg_b, 1) for _ in range(args.repeat)]
            report("dense %d x %d" % (G, n), sizes, ta, tb, agreement)
            del pts
        else:
            raise SystemExit("unknown case %r" % kind)


if __name__ == "__main__":
    main()
