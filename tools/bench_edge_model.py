#!/usr/bin/env python3
"""Times the edge network (`MODEL.TYPE: "EDGEPN2D"`) against the contact network (`"PN2"`), shipped configuration,
`--scenes` x `--points` points.

  (1) FusedPointNet2 f16x2    EDGEPN2D and PN2, ALTERNATING in one process: `--repeat` rounds of `--steps` forwards each
                              between device events; ms / step and scenes / s per network, and the difference
  (2) accelerate()d modules   the edge network, f16x2
  (3) plain torch modules     the edge network (the reference-shaped modules over the HIP operators)
  (4) per launch              one pass of each network under the operator timers: the launches whose time differs

The launch list predicts ONE extra short launch per edge level (`sa{l}.0c`, M rows) and nothing else: the per-point
layer `sa{l}.0f` has the contact network's depth, the chain launch the same shapes.  Both networks are seeded and
calibrated the same way (model.calibrate_bn_ on the timed batch's first two scenes).  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def stats(ms, scenes):
    med = float(np.median(ms))
    return {"rounds": len(ms), "min_ms": round(min(ms), 3), "median_ms": round(med, 3), "max_ms": round(max(ms), 3),
            "scenes_per_s": round(scenes * 1000.0 / med, 1)}


def launch_table(run, batch):
    """{launch name: ms} of one forward pass under the operator timers."""
    from s4g_release_amd import functions as F
    F.OpTimer.reset(True)
    run(batch)
    torch.cuda.synchronize()
    rows = F.OpTimer.summary()                       # {op: (launches, mean ms, bytes, flops)}
    F.OpTimer.reset(False)
    return {name: round(v[0] * v[1], 4) for name, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--points", type=int, default=25600)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--module-steps", type=int, default=2)
    args = ap.parse_args()
    import s4g_release_amd
    from s4g_release_amd import synth
    from s4g_release_amd.fused import FusedPointNet2
    from s4g_release_amd.model import build_model, calibrate_bn_
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_batch(list(range(args.scenes)), args.points)).to(dev)
    batch = {"scene_points": pts}
    nets, runs = {}, {}
    for kind in ("PN2", "EDGEPN2D"):
        torch.manual_seed(11)
        net = build_model(kind).to(dev)
        calibrate_bn_(net, 12, {"scene_points": pts[:2].contiguous()})
        nets[kind] = net.eval()
        runs[kind] = FusedPointNet2(nets[kind], precision="f16x2")
    ms = {k: [] for k in runs}
    for k in runs:                                   # warm-up: lazy kernel attributes, allocator pools
        timed(lambda: runs[k](batch), 2)
    for _ in range(args.repeat):
        for k in runs:
            ms[k].append(timed(lambda: runs[k](batch), args.steps))
    out = {"scenes": args.scenes, "points": args.points, "steps": args.steps,
           "fused_f16x2": {k: stats(v, args.scenes) for k, v in ms.items()}}
    out["fused_f16x2"]["edge_minus_contact_ms"] = round(float(np.median(ms["EDGEPN2D"]) - np.median(ms["PN2"])), 3)
    out["fused_f16x2"]["spreads_overlap"] = not (max(ms["PN2"]) < min(ms["EDGEPN2D"]) or max(ms["EDGEPN2D"]) < min(ms["PN2"]))
    try:
        tabs = {k: launch_table(runs[k], batch) for k in runs}
        names = sorted(set(tabs["PN2"]) | set(tabs["EDGEPN2D"]))
        out["launches_ms"] = {n: [tabs["PN2"].get(n), tabs["EDGEPN2D"].get(n)] for n in names
                              if n.startswith("gemm[sa") or tabs["PN2"].get(n) is None}
    except Exception as e:                           # the timers' interface is not this tool's subject
        out["launches_ms"] = "unavailable: %r" % (e,)
    with torch.no_grad():
        edge = nets["EDGEPN2D"]
        timed(lambda: edge(batch), 1)
        out["modules_torch"] = stats([timed(lambda: edge(batch), args.module_steps) for _ in range(3)], args.scenes)
        s4g_release_amd.accelerate(edge, precision="f16x2")
        timed(lambda: edge(batch), 1)
        out["modules_accelerated_f16x2"] = stats([timed(lambda: edge(batch), args.module_steps) for _ in range(3)],
                                                 args.scenes)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
