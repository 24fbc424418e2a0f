#!/usr/bin/env python3
"""Cost of the contact network's output tail: one forward step of the contact model (`MODEL.TYPE: "PN2"`) against the
curvature model (`"PN2_CLS"`) at 16 x 25 600 points, the same calibrated backbone and heads (tests/golden_util
.calib_full_model; the contact net differs in its two logit layers and the `s4g_contact_heads_f32` launch), the same
process, alternating.  Both forwards are timed as graph replays (the launch sequence without host overhead) and as
eager calls.  Prints one JSON line.

    python tools/contact_step.py [--steps 30] [--warmup 5] [--batch 16]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, steps):
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    from s4g_release_amd import synth
    from s4g_release_amd.fused import FusedPointNet2
    from tests import golden_util as GU
    from tests.contact64 import shipped_contact_net
    dev = torch.device("cuda:0")
    pts = torch.from_numpy(synth.make_batch(list(range(args.batch)), 25600)).to(dev)
    runs = {"PN2_CLS": FusedPointNet2(GU.shipped_net(dev)), "PN2": FusedPointNet2(shipped_contact_net(dev))}
    assert runs["PN2"].kind == "PN2" and runs["PN2_CLS"].kind == "PN2_CLS"
    batch = {"scene_points": pts}
    graphs = {k: r.graph(batch) for k, r in runs.items()}
    res = {}
    with torch.no_grad():
        for mode in ("graph", "eager"):
            fns = {k: ((lambda g=graphs[k]: g(batch)) if mode == "graph" else (lambda r=r: r(batch)))
                   for k, r in runs.items()}
            for k, fn in fns.items():
                _time(fn, args.warmup)
            ms = {k: [] for k in fns}
            for _ in range(args.steps):          # alternate the two networks: drift hits both alike
                for k, fn in fns.items():
                    ms[k] += _time(fn, 1)
            for k in fns:
                res["%s_%s_ms" % (mode, k)] = round(statistics.median(ms[k]), 4)
                res["%s_%s_min_ms" % (mode, k)] = round(min(ms[k]), 4)
            res["%s_overhead_pct" % mode] = round(100.0 * (res["%s_PN2_ms" % mode] / res["%s_PN2_CLS_ms" % mode] - 1), 2)
    res.update(batch=args.batch, points=25600, steps=args.steps, device=torch.cuda.get_device_name(dev))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
