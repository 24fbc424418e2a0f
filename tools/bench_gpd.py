#!/usr/bin/env python3
"""Times the GPD classifier on the close-region maps, in one process:

  (a) baselines.FusedGPD                   csrc/gpd.hip, the frames selected by index inside the loader
  (b) baselines.GPDClassifier in torch     the reference-shaped module on the same device with the same weights, fp32,
                                           after its own warm-up, including the `maps[index]` gather it needs

Inputs (`--sizes`, images per call): real maps = `postprocess.close_regions` on the synthetic scenes of
tools/bench_close_region.py (16 scenes x 512 frames of 200 000 points; the first G frames), and as many dense images
(uniform in [-1, 1)).  Weights: tests/gpd_ref.hashed_state(12, 3).  Method: warm-up, then `--repeat` timings of `--inner`
calls between device events; the median and the spread.  `mfma_tf_issued` counts the fp16 MFMA work the kernels issue
(three products per MAC, padded channels and k-steps included) over the time of the whole call, to be held against the
calibrated loop ceiling of profiles/r05_mfma_ceiling.md (1 248 TF).  `agreement` is the largest distance of (a) from (b)
over the logits' scale.  One JSON line per size and input kind."""
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


def issued_flop_per_image(cin):
    steps1 = (25 * (1 if cin <= 8 else 2) + 1) // 2
    conv1 = 98 * steps1 * 3 * MFMA_FLOP             # 14 x 7 tiles of 32 positions, one channel tile
    conv2 = 18 * 2 * 38 * 3 * MFMA_FLOP             # 6 x 3 tiles, two channel tiles, 38 k-steps
    fc1 = 450 * 16 * 3 * MFMA_FLOP / 32.0           # 32 images per MFMA row tile
    return conv1 + conv2 + fc1


def real_maps(dev, B, N, F):
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
    r = PP.close_regions(torch.from_numpy(G).to(dev), xyz, nrm, PP.LocalSearchConfig(), capacity=F * 8192)
    torch.cuda.synchronize()
    return r.maps.reshape(B * F, 12, 60, 60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 8192])
    ap.add_argument("--scenes", type=int, nargs=3, default=[16, 200000, 512], help="B N F of the scenes the real maps come from")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=None)
    args = ap.parse_args()
    from s4g_release_amd.baselines import FusedGPD, GPDClassifier
    from tests import gpd_ref as GR
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    cin, classes = 12, 3
    net = GPDClassifier(cin, classes)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in GR.hashed_state(cin, classes).items()}, strict=True)
    net = net.to(dev).eval()
    run = FusedGPD(net)
    run.pack(dev)
    B, N, F = args.scenes
    pool = {"real": real_maps(dev, B, N, F)}
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    pool["dense"] = torch.rand(pool["real"].shape, device=dev, generator=gen) * 2 - 1
    for G in args.sizes:
        assert G <= len(pool["real"]), "more images than the scenes hold"
        for kind in ("real", "dense"):
            maps = pool[kind]
            index = torch.arange(G, device=dev)
            index32 = index.int()
            leg_a = lambda: run(maps, index=index32, chunk=args.chunk)                                   # noqa: E731
            with torch.no_grad():
                leg_b = lambda: net({"close_region_projection_maps": maps[index]})["grasp_logits"]      # noqa: E731
                for _ in range(3):
                    got, ref = leg_a(), leg_b()
                torch.cuda.synchronize()
                agreement = float((got - ref).abs().max() / ref.abs().max())
                ta = [timed(leg_a, args.inner) for _ in range(args.repeat)]
                tb = [timed(leg_b, args.inner) for _ in range(args.repeat)]
            a, b = float(np.median(ta)), float(np.median(tb))
            print(json.dumps({
                "G": G, "maps": kind, "occupied_fraction": round(float((maps[:G] != 0).float().mean()), 4),
                "fused_ms": round(a, 3), "fused_min_max_ms": [round(min(ta), 3), round(max(ta), 3)],
                "torch_ms": round(b, 3), "torch_min_max_ms": [round(min(tb), 3), round(max(tb), 3)],
                "fused_images_per_s": round(G / a * 1e3), "torch_images_per_s": round(G / b * 1e3),
                "torch_over_fused": round(b / a, 2),
                "mfma_tf_issued": round(G * issued_flop_per_image(cin) / a * 1e-9, 1),
                "fraction_of_ceiling": round(G * issued_flop_per_image(cin) / a * 1e-9 / CEILING_TF, 3),
                "agreement": agreement}), flush=True)


if __name__ == "__main__":
    main()
