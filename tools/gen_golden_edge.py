#!/usr/bin/env python3
"""Calibrated golden fixture of the EDGE network (`MODEL.TYPE: "EDGEPN2D"`): the reference's own
`network_models/models/EdgePointNet2Down.py` (the contact network with `EdgeSAModule` set abstraction) with BatchNorm
statistics calibrated through its own modules, built the way tools/gen_golden_contact.py builds
pn2_contact_calib_small.npz.

IN-CONTAINER ONLY (imports /root/reference/inference/grasp_proposal/... over the oracle stand-in of `pn2_ext`).
`pointnet2_utils/modules.py` imports `gather_knn` and with it the DGCNN extension `dgcnn_ext`; `EdgeSAModule` never
calls it, so the stub of tools/gen_golden_contact.py satisfies the import.

As there, `t_logit` (zero-initialised by the reference) is RE-SEEDED to offsets of a few cm, and forward hooks on
`R_logit` / `t_logit` store the raw 6-D rotation logits and offsets.  Forward hooks on `sa_modules[i]` store a sampled
slice (FEAT_POS positions x FEAT_CH channels, seeded) of every SA level's feature tensor: the edge term lives in
levels 1 and 2, and a slice pins it there, in front of everything the FP stack and the heads do to it.

  tests/golden/pn2_edge_calib_small.npz  reduced config (tools/gen_golden.SMALL), two scenes of 2 048 points: points,
      the whole state_dict, the four outputs, raw/R6 and raw/t, the index tensors (fps / ball / cnt / nn) of all three
      levels, feat/sa{l} with featpos/sa{l} and featch/sa{l}.
The float64 yardstick is not stored (size): tests form it from the stored weights (tests/edge64.py).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import gen_golden_contact as C  # noqa: E402  (installs the dgcnn_ext stub on import)
from s4g_release_amd import synth  # noqa: E402
from s4g_release_amd.model import calibrate_bn_  # noqa: E402
from tools import gen_golden_calib as G  # noqa: E402
from tools.gen_golden import SMALL, _np, state_dict_sha256  # noqa: E402

HEADS = C.HEADS
T_STD = C.T_STD
FEAT_POS, FEAT_CH = 24, 16
NAME = "pn2_edge_calib_small.npz"


def setup():
    """The reference's EdgePointNet2Down class (imported once, over the oracle stand-in) + the captured index dict."""
    _, captured = G.setup()
    from grasp_proposal.network_models.models.EdgePointNet2Down import EdgePointNet2Down as RefEdge
    return RefEdge, captured


def gen_small(out_dir):
    """tests/golden/pn2_edge_calib_small.npz (a few seconds; tests/test_edge_model.py regenerates and compares)."""
    RefEdge, captured = setup()
    seed = 4323
    torch.manual_seed(seed)
    net = RefEdge(**SMALL)
    assert float(net.t_logit.weight.detach().abs().max()) == 0.0           # the reference's own init
    # edge levels by the first conv's width: level 0 has no features, levels 1 and 2 take 2 C + 3 inputs
    widths = [m.mlp[0].conv.in_channels for m in net.sa_modules]
    assert widths == [3] + [2 * ch[-1] + 3 for ch in SMALL["sa_channels"][:-1]], widths
    g = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        net.t_logit.weight.copy_(torch.randn(net.t_logit.weight.shape, generator=g) * T_STD)
        net.t_logit.bias.copy_(torch.randn(net.t_logit.bias.shape, generator=g) * T_STD)
    pts = synth.make_batch([25, 26], 2048)
    t_pts = torch.from_numpy(pts)
    calibrate_bn_(net, seed + 1, {"scene_points": t_pts}, decades=G.DECADES)
    assert not net.training and not any(m.training for m in net.modules())
    raw, feats = {}, {}
    net.R_logit.register_forward_hook(lambda m, a, out: raw.__setitem__("R6", out))
    net.t_logit.register_forward_hook(lambda m, a, out: raw.__setitem__("t", out))
    for i, m in enumerate(net.sa_modules):
        m.register_forward_hook(lambda mod, a, out, i=i: feats.__setitem__("sa%d" % i, out[1]))
    captured.clear()
    with torch.no_grad():
        pred = net({"scene_points": t_pts})
    sd = net.state_dict()
    assert len(sd) == 200
    blob = {"points": pts, "seed": np.int64(seed), "decades": np.float64(G.DECADES), "t_std": np.float64(T_STD),
            "config_repr": np.array(repr(SMALL)), "state_dict_sha256": np.array(state_dict_sha256(sd))}
    for k, v in sd.items():
        blob["sd/" + k] = _np(v)
    for k in HEADS:
        blob["out/" + k] = _np(pred[k])
    for k, v in raw.items():
        blob["raw/" + k] = _np(v)
    for k in ("scene_score_logits", "frame_R", "movable_logits"):
        G.spread_check("edge/" + k, blob["out/" + k])
    G.spread_check("edge/raw/R6", blob["raw/R6"])
    G.spread_check("edge/raw/t", blob["raw/t"])
    assert np.array_equal(blob["out/frame_t"], (t_pts + raw["t"]).numpy())
    rng = np.random.default_rng(seed + 3)
    for lv in sorted(feats):
        a = _np(feats[lv])                               # (2, C, M)
        G.spread_check("edge/feat/" + lv, a, strict=False)
        pos = np.sort(rng.choice(a.shape[2], FEAT_POS, replace=False)).astype(np.int64)
        ch = np.sort(rng.choice(a.shape[1], FEAT_CH, replace=False)).astype(np.int64)
        blob["featpos/" + lv], blob["featch/" + lv] = pos, ch
        blob["feat/" + lv] = np.ascontiguousarray(a[:, ch][:, :, pos])
    for li, r in enumerate(captured["farthest_point_sample"]):
        blob["fps%d" % li] = _np(r)
    for li, (i, c) in enumerate(captured["ball_query"]):
        blob["ball%d" % li] = _np(i).astype(np.int32)
        blob["cnt%d" % li] = _np(c).astype(np.int32)
    for li, (i, d) in enumerate(captured["point_search"]):
        blob["nn%d" % li] = _np(i).astype(np.int32)
    path = os.path.join(out_dir, NAME)
    np.savez_compressed(path, **blob)
    print("%s: %d bytes" % (os.path.basename(path), os.path.getsize(path)))


def main():
    gen_small(os.environ.get("S4G_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden")))


if __name__ == "__main__":
    main()
