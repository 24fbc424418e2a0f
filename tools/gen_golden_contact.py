#!/usr/bin/env python3
"""Calibrated golden fixture of the CONTACT network (`MODEL.TYPE: "PN2"`): the reference's own
`network_models/models/PointNet2.py` with BatchNorm statistics calibrated through its own modules, built the way
tools/gen_golden_calib.py builds pn2_calib_small.npz.

IN-CONTAINER ONLY (imports /root/reference/inference/grasp_proposal/... over the oracle stand-in of `pn2_ext`, as
tools/gen_golden_calib.py does).  `PointNet2.py` imports `functions/functions.py` (for `toRotMatrix`), which imports
the DGCNN extension `dgcnn_ext`; the contact network never calls it, so a stub module satisfies the import.

The reference zero-initialises `t_logit` (PointNet2.py:149-152): with that, frame_t == scene_points and the
translation head would go untested, so it is RE-SEEDED to non-zero weights here (std T_STD, offsets of a few cm).
A forward hook on `R_logit` / `t_logit` stores the raw 6-D rotation logits and the raw offsets, so that tests can
tell the conditioning of the 6-D -> matrix map from an error of the backbone.

  tests/golden/pn2_contact_calib_small.npz  reduced config (tools/gen_golden.SMALL), two scenes of 2 048 points:
      points, the whole state_dict, the four outputs (scene_score_logits / frame_R / frame_t / movable_logits),
      raw/R6 and raw/t, and the index tensors (fps / ball / cnt / nn) of all three levels.
The float64 yardstick is not stored (size): tests form it from the stored weights (tests/contact64.py).
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DGCNN = "grasp_proposal.network_models.functions.dgcnn_ext"


def _install_dgcnn_stub():
    """`functions/gather_knn.py` imports the DGCNN extension (before tools.gen_golden imports the reference tree)."""
    if DGCNN not in sys.modules:
        stub = types.ModuleType(DGCNN)

        def _unused(*a):
            raise RuntimeError("dgcnn_ext is not used by the contact network")
        stub.gather_knn_forward = stub.gather_knn_backward = _unused
        sys.modules[DGCNN] = stub


_install_dgcnn_stub()

from s4g_release_amd import synth  # noqa: E402
from s4g_release_amd.model import calibrate_bn_  # noqa: E402
from tools import gen_golden_calib as G  # noqa: E402
from tools.gen_golden import SMALL, _np, state_dict_sha256  # noqa: E402

HEADS = ("scene_score_logits", "frame_R", "frame_t", "movable_logits")
T_STD = 0.01


def setup():
    """The reference's contact PointNet2 class (imported once, over the oracle stand-in) + the captured index dict."""
    _, captured = G.setup()                        # stand-in pn2_ext, reference tree on sys.path, index capture
    from grasp_proposal.network_models.models.PointNet2 import PointNet2 as RefContact
    return RefContact, captured


def gen_small(out_dir):
    """tests/golden/pn2_contact_calib_small.npz (a few seconds; tests/test_contact_model.py regenerates and compares)."""
    RefContact, captured = setup()
    seed = 4322
    torch.manual_seed(seed)
    net = RefContact(**SMALL)
    assert float(net.t_logit.weight.detach().abs().max()) == 0.0           # the reference's own init
    g = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        net.t_logit.weight.copy_(torch.randn(net.t_logit.weight.shape, generator=g) * T_STD)
        net.t_logit.bias.copy_(torch.randn(net.t_logit.bias.shape, generator=g) * T_STD)
    pts = synth.make_batch([23, 24], 2048)
    t_pts = torch.from_numpy(pts)
    calibrate_bn_(net, seed + 1, {"scene_points": t_pts}, decades=G.DECADES)
    assert not net.training and not any(m.training for m in net.modules())
    raw = {}
    net.R_logit.register_forward_hook(lambda m, a, out: raw.__setitem__("R6", out))
    net.t_logit.register_forward_hook(lambda m, a, out: raw.__setitem__("t", out))
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
    # per-point spread: the outputs, the raw 6-D logits and the raw offsets (frame_t's spread is the points')
    for k in ("scene_score_logits", "frame_R", "movable_logits"):
        G.spread_check("contact/" + k, blob["out/" + k])
    G.spread_check("contact/raw/R6", blob["raw/R6"])
    G.spread_check("contact/raw/t", blob["raw/t"])
    assert np.array_equal(blob["out/frame_t"], (t_pts + raw["t"]).numpy())
    for li, r in enumerate(captured["farthest_point_sample"]):
        blob["fps%d" % li] = _np(r)
    for li, (i, c) in enumerate(captured["ball_query"]):
        blob["ball%d" % li] = _np(i).astype(np.int32)
        blob["cnt%d" % li] = _np(c).astype(np.int32)
    for li, (i, d) in enumerate(captured["point_search"]):
        blob["nn%d" % li] = _np(i).astype(np.int32)
    path = os.path.join(out_dir, "pn2_contact_calib_small.npz")
    np.savez_compressed(path, **blob)
    print("%s: %d bytes" % (os.path.basename(path), os.path.getsize(path)))


def main():
    gen_small(os.environ.get("S4G_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden")))


if __name__ == "__main__":
    main()
