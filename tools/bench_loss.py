#!/usr/bin/env python3
"""Times the fused training objective (`losses.PointNet2Loss` / `ContactPointNet2Loss`: one `s4g_grasp_loss_f32` call)
against the reference-shaped loss in plain torch operations (the restatement of tests/test_loss_gpu.py; its class
weights made once, outside: the reference writes them from the host in every forward, which no capture takes) on the
same device and inputs, forward + backward to the prediction gradients, in one process:

  fused / torch               eager: forward, `sum(losses).backward()`;
  fused_graph / torch_graph   the same captured once and replayed;
  call_graph                  the three launches of `s4g_grasp_loss_f32` alone (losses and the four unit gradients),
                              replayed: what the traffic figure is taken of.

Shape: `--scenes` scenes of `--points` points, `--frames` frame points (default 16 x 25 600, F = 2 048), both variants.
Method: every leg warmed up, then `--repeat` rounds of `--inner` calls between device events, the legs in alternating
order; the median and the (min, max) per leg.  Launches per leg are counted from a profiler trace of one eager call
(None where the profiler gives no kernel events).  One JSON line per variant, and with `--out FILE` the table that
profiles/r29_loss.md quotes."""
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


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def captured(fn, dev):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--points", type=int, default=25600)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import s4g_release_amd as S
    from tests import loss_ref as LR
    from tests import test_loss_gpu as TG
    assert torch.cuda.is_available(), "a timing needs the GPU"
    assert args.repeat >= 5, "at least five rounds"
    dev = torch.device("cuda:0")
    B, N, F = args.scenes, args.points, args.frames
    rows = []
    for model_type, variant in (("PN2_CLS", LR.CURVATURE), ("PN2", LR.CONTACT)):
        preds, labels = LR.random_case(29, variant, B, N, F, stride=F + 8)
        p = {TG.PRED_KEYS[k]: torch.from_numpy(v).to(dev).requires_grad_() for k, v in preds.items()}
        lab = {TG.LABEL_KEYS[k]: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in labels.items()}
        fused_loss = S.build_loss(model_type)[0]

        def step(loss_of):
            for v in p.values():
                v.grad = None
            sum(loss_of().values()).backward()
        fused = lambda: step(lambda: fused_loss(p, lab))                                   # noqa: E731
        consts = TG._torch_constants(preds["score"].shape[1], fused_loss.neg_weight, dev)
        plain = lambda: step(lambda: TG._torch_loss(variant, p, lab, fused_loss.neg_weight, consts))   # noqa: E731
        call = TG._Call(dev, variant, preds, labels, 0.0, fused_loss.neg_weight)
        fused()
        g_fused = {k: v.grad.clone() for k, v in p.items()}
        plain()
        worst = max(float((v.grad - g_fused[k]).abs().max() / v.grad.abs().max()) for k, v in p.items())
        launches = {"fused": count_launches(fused), "torch": count_launches(plain), "call_graph": count_launches(call.launch)}
        graphs = {"fused_graph": captured(fused, dev), "torch_graph": captured(plain, dev),
                  "call_graph": captured(call.launch, dev)}
        legs = {"fused": fused, "torch": plain}
        legs.update({k: g.replay for k, g in graphs.items()})
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in legs}
        for i in range(args.repeat):
            for k in (list(legs) if i % 2 == 0 else list(legs)[::-1]):
                t[k].append(timed(legs[k], args.inner))
        med = {k: float(np.median(v)) for k, v in t.items()}
        pred_bytes = sum(v.size * 4 for v in preds.values())
        label_bytes = sum(v.nbytes for v in labels.values())
        row = {"model_type": model_type, "B": B, "N": N, "F": F, "launches": launches,
               "pred_bytes": pred_bytes, "label_bytes": label_bytes, "fused_vs_torch_gradient": worst,
               "call_bytes_per_s": (2 * pred_bytes + label_bytes) / (med["call_graph"] * 1e-3)}
        for k in legs:
            row[k + "_ms"] = round(med[k], 4)
            row[k + "_min_max_ms"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if not args.out:
        return
    with open(args.out, "w") as f:
        f.write("# The fused loss against the plain-torch loss (tools/bench_loss.py)\n\n")
        f.write("%d scenes of %d points, F = %d, forward + backward to the prediction gradients.  Median of %d rounds of %d\n"
                "calls between device events, legs alternating, (min, max) in brackets; launches from a profiler trace of\n"
                "one eager call.\n\n" % (B, N, F, args.repeat, args.inner))
        f.write("| model | leg | ms | launches |\n|---|---|---|---|\n")
        for r in rows:
            for k in ("fused", "torch", "fused_graph", "torch_graph", "call_graph"):
                f.write("| %s | %s | %.4f (%.4f, %.4f) | %s |\n" % (r["model_type"], k, r[k + "_ms"], *r[k + "_min_max_ms"],
                                                               r["launches"].get(k.replace("_graph", "") if k != "call_graph" else k)))
        f.write("\n")
        for r in rows:
            f.write("%s: the call alone moves %.1f MB of predictions, as many of gradients and %.1f MB of labels in %.4f ms: "
                    "%.2f TB/s.  Largest gradient difference between the two losses: %.2g of the tensor's largest gradient.\n"
                    % (r["model_type"], r["pred_bytes"] / 1e6, r["label_bytes"] / 1e6, r["call_graph_ms"],
                       r["call_bytes_per_s"] / 1e12, r["fused_vs_torch_gradient"]))
    print(args.out)


if __name__ == "__main__":
    main()
