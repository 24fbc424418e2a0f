"""Time the reference-shaped modules path three ways in ONE process, with device events: the torch modules path
(conv / BatchNorm / ReLU / torch.max), the same network after `s4g_release_amd.accelerate(net)` at f16x2 and at
fp32.  Workload: B tabletop-v1 scenes of N points (default 16 x 25 600), the calibrated shipped network
(tests/golden/pn2_calib_full.npz), warm-up first, the paths alternated step by step.

--ab adds the channels-first loader's kill-criterion A/B at SA-level-2 size (16 x 1 024 x 64 rows, Cin = 259 ->
256, f16x2): the loader reading (B, Cin, L) directly against a channels-last transpose (torch copy into a
4-aligned (P, 260) buffer) followed by the PLAIN loader.

Prints one JSON line."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _time(fn, reps, torch):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def ab_loader(torch, dev, reps):
    from s4g_release_amd import accelerated as A
    from s4g_release_amd.fused import _Layer, _pad_k
    B, M, K, cin, cout = 16, 1024, 64, 259, 256
    L, P = M * K, B * M * K
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(dev)
    layer = _Layer(_pad_k(w), torch.zeros(cout, device=dev), cin)
    x = torch.randn(B, cin, L, device=dev)
    amax = A._amax(x, B)
    out = torch.empty((P, cout), device=dev)
    xt = torch.zeros((P, 260), device=dev)
    prec = A.PRECISIONS["f16x2"]

    def cf():
        A._launch(layer, prec, True, A.LOAD_CHANNEL_FIRST, A.EPI_STORE, P, cin, x, out, L, a_L=L, a_amax=amax,
                  ldc=cout)

    def transpose_plain():
        xt.view(B, L, 260)[:, :, :cin].copy_(x.permute(0, 2, 1))
        A._launch(layer, prec, True, A.LOAD_PLAIN, A.EPI_STORE, P, 260, xt, out, L, lda=260, a_amax=amax, ldc=cout)

    def plain_only():
        A._launch(layer, prec, True, A.LOAD_PLAIN, A.EPI_STORE, P, 260, xt, out, L, lda=260, a_amax=amax, ldc=cout)

    res = {}
    for _ in range(2):                       # alternate, keep the best of two rounds
        for name, fn in (("channel_first_loader", cf), ("transpose_plus_plain", transpose_plain),
                         ("plain_alone", plain_only)):
            fn()
            t = _time(fn, reps, torch)
            res[name] = min(res.get(name, t), t)
    cf()
    a = out.clone()
    transpose_plain()
    res["max_abs_diff"] = float((a - out).abs().max())
    return {k + ("_ms" if k != "max_abs_diff" else ""): round(v, 4) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=25600)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--paths", default="torch,f16x2,fp32")
    ap.add_argument("--ab", action="store_true")
    args = ap.parse_args()
    import torch
    import s4g_release_amd
    from s4g_release_amd import synth
    from tests import golden_util as GU
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda:0")
    base = GU.calib_full_model().to(dev).eval()
    pts = torch.from_numpy(synth.make_batch(list(range(args.batch)), args.points)).to(dev)
    batch = {"scene_points": pts}
    nets = {}
    for name in args.paths.split(","):
        net = copy.deepcopy(base)
        if name != "torch":
            s4g_release_amd.accelerate(net, precision=name)
        nets[name] = net
    times = {n: [] for n in nets}
    outs = {}
    with torch.no_grad():
        for _ in range(args.warmup):
            for n, net in nets.items():
                outs[n] = net(batch)
        torch.cuda.synchronize()
        for _ in range(args.steps):
            for n, net in nets.items():
                times[n].append(_time(lambda: net(batch), 1, torch))
    ms = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
    res = {"metric": "modules_path_scenes_per_s", "batch": args.batch, "points": args.points, "steps": args.steps,
           "step_ms_median": {n: round(v, 3) for n, v in ms.items()},
           "scenes_per_s": {n: round(1000.0 * args.batch / v, 1) for n, v in ms.items()}}
    if "torch" in ms:
        res["speedup_vs_torch"] = {n: round(ms["torch"] / v, 3) for n, v in ms.items() if n != "torch"}
        ref = outs["torch"]
        res["max_rel_diff_vs_torch"] = {
            n: max(float((o[k] - ref[k]).abs().max()) / max(1.0, float(ref[k].abs().max())) for k in ref)
            for n, o in outs.items() if n != "torch"}
    if args.ab:
        with torch.no_grad():
            res["loader_ab_sa2"] = ab_loader(torch, dev, 10)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
