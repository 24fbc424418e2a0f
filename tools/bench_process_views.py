#!/usr/bin/env python3
"""Times `preprocess.process_views` (crop, voxel trace, radius outliers of B views in one sync-free call) against the
way the same result was made before it existed, in one process on the same inputs:

  batched   `process_views(clouds)`, eager;
  graph     the same call captured once and replayed;
  loop      per view `filter_work_space` -> `voxel_down_sample` -> `radius_outlier_mask` and the final gather, with
            their host reads (a count per crop and per voxel call, the cloud's bounds per voxel call).

Shapes: `--views` table-top views (`synth`) of `--points` rows each (default 16 and 1 views of 48 902 rows, the size of
a rendered view after the depth mask), lifted into the camera frame so that the generator's workspace holds the table;
the data generator's constants (`ViewProcessingConfig`).  Method: every leg warmed up, then `--repeat` rounds of
`--inner` calls between device events, the legs in alternating order; the median and the (min, max) per leg.  The loop
leg ends in host reads, so its events close after them.  One JSON line per shape, and the table of `--out` (default
profiles/r25_process_views.md).  `--calls K` runs the batched call K times and nothing else: the run a kernel trace
is taken of."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAMERA_LIFT = 2.145          # synth's table top to just above the workspace's floor (0.749)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def make_views(B, N, dev):
    from s4g_release_amd import synth
    x = synth.make_batch(list(range(B)), N).astype(np.float32)
    x[:, 2] += np.float32(CAMERA_LIFT)
    return torch.from_numpy(x).to(dev)


def loop_leg(PP, x, cfg):
    """The parent's way, view after view -> [(3, K_b) tensors]."""
    out = []
    for b in range(x.size(0)):
        kept = PP.filter_work_space(x[b], cfg.workspace)
        means = PP.voxel_down_sample(x[b][:, kept].contiguous(), cfg.voxel_size)
        out.append(means[:, PP.radius_outlier_mask(means, cfg.nb_points, cfg.radius)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[16, 1])
    ap.add_argument("--points", type=int, default=48902)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_process_views.md"))
    args = ap.parse_args()
    from s4g_release_amd import preprocess as PP
    assert torch.cuda.is_available(), "a timing needs the GPU"
    assert args.repeat >= 5, "at least five rounds"
    dev = torch.device("cuda:0")
    cfg = PP.ViewProcessingConfig()
    if args.calls:
        x = make_views(args.views[0], args.points, dev)
        for _ in range(args.calls):
            PP.process_views(x, None, cfg)
        torch.cuda.synchronize()
        return
    rows = []
    for B in args.views:
        x = make_views(B, args.points, dev)
        batched = lambda: PP.process_views(x, None, cfg)                    # noqa: E731
        first = batched()
        old = loop_leg(PP, x, cfg)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            batched()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = batched()
        graph.replay()
        torch.cuda.synchronize()
        same_graph = bool(torch.equal(captured.index_in_ref, first.index_in_ref) and
                          torch.equal(captured.count, first.count))
        # the loop's voxel grid starts at each cloud's own minimum, so its cells are not the generator's: the kept
        # counts are comparable, the points are not
        counts = first.count.cpu().tolist()
        legs = {"batched": batched, "graph": graph.replay, "loop": lambda: loop_leg(PP, x, cfg)}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for i in range(args.repeat):
            for k in (list(legs) if i % 2 == 0 else list(legs)[::-1]):
                t[k].append(timed(legs[k], args.inner))
        med = {k: float(np.median(v)) for k, v in t.items()}
        row = {"B": B, "N": args.points, "crop_count": first.crop_count.cpu().tolist()[:4],
               "voxel_count": first.voxel_count.cpu().tolist()[:4], "count": counts[:4],
               "loop_count": [int(o.size(1)) for o in old][:4], "graph_equals_eager": same_graph}
        for k in legs:
            row[k + "_ms"] = round(med[k], 3)
            row[k + "_min_max_ms"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
        row["loop_over_batched"] = round(med["loop"] / med["batched"], 3)
        row["loop_over_graph"] = round(med["loop"] / med["graph"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, first, old, captured, graph
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("# process_views against the per-view loop it replaces (tools/bench_process_views.py)\n\n")
        f.write("Table-top views of %d rows in the camera frame, the data generator's constants (crop, voxel 0.005 over\n"
                "201 x 201 x 161 cells, radius 0.04 with more than 8 neighbours).  `loop` is per view\n"
                "`filter_work_space` -> `voxel_down_sample` -> `radius_outlier_mask` with their host reads.  Median of %d\n"
                "rounds of %d calls between device events, legs alternating, (min, max) in brackets.\n\n"
                % (args.points, args.repeat, args.inner))
        f.write("| views | batched ms | replayed graph ms | per-view loop ms | loop / batched | loop / graph |\n")
        f.write("|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %d | %.3f (%.3f, %.3f) | %.3f (%.3f, %.3f) | %.3f (%.3f, %.3f) | %.2f | %.2f |\n"
                    % (r["B"], r["batched_ms"], *r["batched_min_max_ms"], r["graph_ms"], *r["graph_min_max_ms"],
                       r["loop_ms"], *r["loop_min_max_ms"], r["loop_over_batched"], r["loop_over_graph"]))
        f.write("\nRows after the crop, voxels and kept means of the first views: "
                + "; ".join("%d views: %s, %s, %s" % (r["B"], r["crop_count"], r["voxel_count"], r["count"]) for r in rows)
                + ".\n")
    print(args.out)


if __name__ == "__main__":
    main()
