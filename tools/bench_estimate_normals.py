#!/usr/bin/env python3
"""Times the normal estimation (`postprocess.estimate_normals`) and, in the same process on the same inputs,
`postprocess.match_normals(cloud, cloud, normals)`: the same grid build and the same hybrid search over the same
candidates, which ends in a mean of the kept normals where the estimation gathers the kept points, sums nine moments and
solves a 3x3 eigenproblem in double.  Their difference is therefore what the moments and the eigen-solve (and the
origin kernel) cost; their ratio is recorded.  Also: the build alone (`count` = 1 live point per scene: the query
kernel has one row to do), and the fixture's cases on this device against their bound (tests/test_normals_gpu.py).

Shapes: `--scenes` clouds of each size in `--points` (default 16 x 25 600 and 16 x 200 000), the table-top scenes of
tools/bench_match_normals.py (cylinders sampled at about 90 points per 1 cm ball, the rest on the table).  Method:
warm-up, then `--repeat` rounds of `--inner` calls between device events, the legs in alternating order; the median
and the spread per leg.  One JSON line per size, and the table of `--out` (default profiles/r19_estimate_normals.md)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_match_normals import make_scene, timed  # noqa: E402


def fixture_on_device(dev):
    """-> per fixture case (margin, worst error / bound, rows judged) on this device."""
    from s4g_release_amd import postprocess as PP
    from tests import golden_util as GU
    from tests import normals_ref as NR
    fx = GU.load("normals.npz")
    out = {}
    for name in ("r10", "r15", "lattice", "sphere"):
        pre = name + "/" if name in ("lattice", "sphere") else ""
        y = {k: fx["%s/%s" % (name, k)] for k in ("normals", "count", "flags", "gap", "towards")}
        margin = float(fx[name + "/margin"][0])
        e = PP.estimate_normals(torch.from_numpy(fx[pre + "cloud"]).to(dev), torch.from_numpy(fx[pre + "camera"]).to(dev),
                                float(fx[name + "/radius"][0]), int(fx[name + "/max_nn"][0]))
        got = e.normals[0].t().cpu().numpy().astype(np.float64)
        judged = (y["count"] >= NR.FEW_BELOW) & (y["gap"] >= 1e-3)
        ratio = NR.row_error(got, y)[judged] / NR.bound(y, margin)[judged]
        exact = bool(np.array_equal(e.count[0].cpu().numpy(), y["count"]) and
                     np.array_equal(e.flags[0].cpu().numpy(), y["flags"]))
        out[name] = {"margin": margin, "worst_error_over_bound": float(ratio.max()), "rows_judged": int(judged.sum()),
                     "count_and_flags_exact": exact}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--points", type=int, nargs="+", default=[25600, 200000])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_estimate_normals.md"))
    args = ap.parse_args()
    from s4g_release_amd import postprocess as PP
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    radius, max_nn = PP.NORMAL_RADIUS, PP.NORMAL_MAX_NN
    th = PP.LocalSearchConfig().table_height
    B = args.scenes
    fixture = fixture_on_device(dev)
    print(json.dumps({"fixture": fixture}), flush=True)
    rows = []
    for N in args.points:
        rng = np.random.default_rng(N)
        scenes = [make_scene(rng, N, 1, th) for _ in range(B)]
        pts, nrm = (torch.from_numpy(np.stack([s[i] for s in scenes])).to(dev) for i in range(2))
        cam = torch.tensor([0.9, -0.3, th + 0.8], device=dev)
        one = torch.ones(B, dtype=torch.int32, device=dev)
        legs = {"estimate": lambda: PP.estimate_normals(pts, cam, radius, max_nn),
                "match": lambda: PP.match_normals(pts, pts, nrm, cam, radius, max_nn),
                "build": lambda: PP.estimate_normals(pts, cam, radius, max_nn, count=one)}
        e = legs["estimate"]()
        m = legs["match"]()
        legs["build"]()
        torch.cuda.synchronize()
        same_sets = bool(torch.equal(e.count, m.count) and torch.equal(e.capped, m.capped))
        t = {k: [] for k in legs}
        for i in range(args.repeat):
            for k in (list(legs) if i % 2 == 0 else list(legs)[::-1]):
                t[k].append(timed(legs[k], args.inner))
        med = {k: float(np.median(x)) for k, x in t.items()}
        spread = {k: [round(min(x), 3), round(max(x), 3)] for k, x in t.items()}
        row = {"B": B, "N": N, "radius": radius, "max_nn": max_nn,
               "estimate_normals_ms": round(med["estimate"], 3), "estimate_normals_min_max_ms": spread["estimate"],
               "match_normals_ms": round(med["match"], 3), "match_normals_min_max_ms": spread["match"],
               "estimate_over_match": round(med["estimate"] / med["match"], 3),
               "moments_and_solve_ms": round(med["estimate"] - med["match"], 3),
               "one_live_point_ms": round(med["build"], 3), "one_live_point_min_max_ms": spread["build"],
               "points_per_second": round(B * N / (med["estimate"] * 1e-3)),
               "the_same_counts_as_match_normals": same_sets, "kept_median": float(e.count.float().median()),
               "capped": int(e.capped.sum()), "few": int(e.few.sum()), "degenerate": int(e.degenerate.sum())}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del pts, nrm, e, m
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("# estimate_normals against match_normals on the same inputs (tools/bench_estimate_normals.py)\n\n")
        f.write("`match_normals(cloud, cloud, normals)` builds the same grid and runs the same hybrid search; the\n"
                "difference of the two calls is what gathering the kept points, the nine moments, the eigen-solve in\n"
                "double and the origin kernel cost.  Median of %d rounds of %d calls between device events, (min, max)\n"
                "in brackets.  radius %g, max_nn %d.\n\n" % (args.repeat, args.inner, radius, max_nn))
        f.write("| B x N | estimate_normals ms | match_normals ms | ratio | difference ms | one live point ms | points / s |\n")
        f.write("|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %d x %d | %.3f (%.3f, %.3f) | %.3f (%.3f, %.3f) | %.3f | %.3f | %.3f | %.3g |\n"
                    % (r["B"], r["N"], r["estimate_normals_ms"], *r["estimate_normals_min_max_ms"], r["match_normals_ms"],
                       *r["match_normals_min_max_ms"], r["estimate_over_match"], r["moments_and_solve_ms"],
                       r["one_live_point_ms"], r["points_per_second"]))
        f.write("\nKept neighbours (median), capped, few and degenerate rows per shape: "
                + "; ".join("%d x %d: %g, %d, %d, %d" % (r["B"], r["N"], r["kept_median"], r["capped"], r["few"],
                                                        r["degenerate"]) for r in rows) + ".\n\n")
        f.write("## The fixture on this device (tests/golden/normals.npz)\n\n")
        f.write("| case | margin | worst error / bound (bound = 8 * margin / g) | rows judged | count and flags exact |\n")
        f.write("|---|---|---|---|---|\n")
        for name, v in fixture.items():
            f.write("| %s | %.3g | %.3g | %d | %s |\n" % (name, v["margin"], v["worst_error_over_bound"], v["rows_judged"],
                                                       v["count_and_flags_exact"]))
    print(args.out)


if __name__ == "__main__":
    main()
